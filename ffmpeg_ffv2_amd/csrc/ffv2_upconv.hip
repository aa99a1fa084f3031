// ffv2_upconv.hip -- 4:2:0 -> 4:4:4 in front of the T-stage.
//
// ffv2's encode2() takes 4:4:4 planar only (ffv2enc.c:596-601); handed a yuv420p* source the
// reference tool chain converts first: choose_pixel_fmt() (fftools/ffmpeg_filter.c:63-131) picks
// yuv444p* of the same depth and libavfilter inserts a scale filter with the tool's default
// flags=bicubic.  With equal luma size that is, in libswscale's generic C scaler:
//   luma    unscaled, filter size 1: the identity;
//   chroma  2x up both ways with the 4-tap bicubic (B = 0, C = 0.6) of initFilter()
//           (libswscale/utils.c:332-727) at sample positions 128/128 (get_local_pos, :303-310;
//           vf_scale.c:566-577), 14-bit horizontal and 12-bit vertical coefficients:
//             h = min((sum_k src[r][hpos[x]+k] * hf[x][k]) >> (8-bit: 7 | deeper: depth-1), 32767)
//                                                               swscale.c:96-139
//             out = clip((round + sum_j h[vpos[y]+j][x] * vf[y][j]) >> shift)
//                   8 bit: round = 64 << 12, shift 19 (yuv2planeX_8_c, no dither for 8-bit sources)
//                   deeper: round = 1 << (shift-1), shift = 27 - depth   (output.c:333-393)
// PARITY UNPINNED: no libswscale binary or vector exists here; checked against
// oracle/ffv2_swscale_oracle.c.  build_axis() below RESTATES initFilter()'s integer steps (they must
// be the same steps for the tables to be bit-exact), and so does the oracle: the coefficient tables
// are effectively compared with a second writing of the same derivation, only the device arithmetic
// of the two 4-tap passes is checked independently.
//
// Host part: the coefficient tables (integer arithmetic of initFilter, once per geometry).
// Device part: ffv2_upconv_tile_kernel -- a workgroup owns a 128 x 32 tile of one output chroma
// plane: the source patch it needs (<= 24 x 80 samples) goes to LDS, the horizontal pass runs once
// per source row into a 15-bit LDS intermediate (what swscale keeps between its two passes), the
// vertical pass reads it back as 16-byte rows and stores 8 samples per lane.  6.4 multiplies per
// output sample instead of the 20 of the one-thread-per-sample kernel, which stays as the fallback
// for geometries whose patch would not fit.  Luma is the identity: rows copied (or, in the frame
// ring, sent by the DMA engine straight into plane 0).
#include "ffv2_kernels.h"

#include <stdlib.h>
#include <vector>

namespace {

constexpr int UP_TAPS = 8;                 // table stride; a 2x bicubic needs 4

// ---- initFilter(), SWS_BICUBIC branch, default parameters, no src/dst filter vectors, C-code
// alignment (1) -- utils.c line numbers in the comments ----
struct AxisFilter {
    int taps = 0;
    std::vector<int16_t> coef;             // [n][UP_TAPS]
    std::vector<int32_t> pos;              // [n]
};

int ilog2u(unsigned v) { int n = 0; while (v >>= 1) n++; return n; }
int64_t iabs64(int64_t v) { return v < 0 ? -v : v; }

bool build_axis(AxisFilter &out, int n, int one)
{
    const int srcN = (n + 1) >> 1;                                            // :1409-1410
    const int inc = (int)((((int64_t)srcN << 16) + (n >> 1)) / n);            // :1443-1444
    const int srcPos = 128, dstPos = 128;                                     // :303-310
    const int64_t fone = 1LL << (54 - (ilog2u((unsigned)(srcN / n)) < 8 ? ilog2u((unsigned)(srcN / n)) : 8));   // :345
    std::vector<int64_t> f;
    std::vector<int32_t> pos((size_t)n);
    int size;
    if (abs(inc - 0x10000) < 10 && srcPos == dstPos) {                        // :355 (n == 1)
        size = 1;
        f.assign((size_t)n, fone);
        for (int i = 0; i < n; i++) pos[(size_t)i] = i;
    } else {
        size = inc <= 1 << 16 ? 1 + 4 : 1 + (4 * srcN + n - 1) / n;           // :418-421, size factor 4
        if (size > srcN - 2) size = srcN - 2;                                 // :423-424
        if (size < 1) size = 1;
        f.resize((size_t)n * size);
        const int64_t C = (int64_t)(0.6 * (1 << 24));                         // :447, B = 0
        int64_t at = ((dstPos * (int64_t)inc) >> 7) - ((srcPos * 0x10000LL) >> 7);   // :429
        for (int i = 0; i < n; i++) {
            int xx = (int)((at - (size - 2) * (1LL << 16)) / (1 << 17));      // :431
            pos[(size_t)i] = xx;
            for (int j = 0; j < size; j++, xx++) {
                int64_t d = iabs64((int64_t)xx * (1 << 17) - at) << 13;       // :435
                if (inc > 1 << 16) d = d * n / srcN;
                int64_t c = 0;
                if (d < 1LL << 31) {
                    const int64_t dd = (d * d) >> 30, ddd = (dd * d) >> 30;
                    c = d < 1LL << 30
                        ? (12 * (1 << 24) - 6 * C) * ddd + (-18 * (1 << 24) + 6 * C) * dd + (6 * (1 << 24)) * (1LL << 30)
                        : (-6 * C) * ddd + (30 * C) * dd + (-48 * C) * d + (24 * C) * (1LL << 30);      // :452-464
                }
                f[(size_t)i * size + j] = c / ((1LL << 54) / fone);           // :466
            }
            at += 2 * inc;
        }
    }
    // shrink: drop near-zero taps on the left (shifting the row), count them on the right  :545-584
    int need = 0;
    for (int i = n - 1; i >= 0; i--) {
        int64_t *row = &f[(size_t)i * size];
        int64_t cut = 0;
        for (int j = 0; j < size; j++) {
            cut += iabs64(row[0]);
            if ((double)cut > 0.002 * (double)fone) break;                    // SWS_MAX_REDUCE_CUTOFF
            if (i < n - 1 && pos[(size_t)i] >= pos[(size_t)i + 1]) break;     // keep positions monotone
            for (int k = 1; k < size; k++) row[k - 1] = row[k];
            row[size - 1] = 0;
            pos[(size_t)i]++;
        }
        int keep = size;
        cut = 0;
        for (int j = size - 1; j > 0; j--) {
            cut += iabs64(row[j]);
            if ((double)cut > 0.002 * (double)fone) break;
            keep--;
        }
        if (keep > need) need = keep;
    }
    if (need < 1 || need > UP_TAPS) return false;
    std::vector<int64_t> g((size_t)n * need);                                 // :617-627
    for (int i = 0; i < n; i++)
        for (int j = 0; j < need; j++) g[(size_t)i * need + j] = j < size ? f[(size_t)i * size + j] : 0;
    // borders: taps that would read outside are folded onto the edge sample  :630-671
    for (int i = 0; i < n; i++) {
        int64_t *row = &g[(size_t)i * need];
        int32_t &p = pos[(size_t)i];
        if (p < 0) {
            for (int j = 1; j < need; j++) {
                const int left = j + p > 0 ? j + p : 0;
                row[left] += row[j];
                row[j] = 0;
            }
            p = 0;
        }
        if (p + need > srcN) {
            const int shift = p + (need - srcN < 0 ? need - srcN : 0);
            int64_t acc = 0;
            for (int j = need - 1; j >= 0; j--)
                if (p + j >= srcN) { acc += row[j]; row[j] = 0; }
            for (int j = need - 1; j >= 0; j--) row[j] = j < shift ? 0 : row[j - shift];
            p -= shift;
            row[srcN - 1 - p] += acc;
        }
    }
    // normalise each row to `one` with error feedback  :679-698
    out.taps = need;
    out.pos = pos;
    out.coef.assign((size_t)n * UP_TAPS, 0);
    for (int i = 0; i < n; i++) {
        const int64_t *row = &g[(size_t)i * need];
        int64_t sum = 0, err = 0;
        for (int j = 0; j < need; j++) sum += row[j];
        sum = (sum + one / 2) / one;
        if (!sum) sum = 1;
        for (int j = 0; j < need; j++) {
            const int64_t v = row[j] + err;
            const int64_t q = (v >= 0 ? v + (sum >> 1) : v - (sum >> 1)) / sum;       // ROUNDED_DIV
            out.coef[(size_t)i * UP_TAPS + j] = (int16_t)q;
            err = v - q * sum;
        }
    }
    return true;
}

struct UpArgs {
    const uint8_t *src;        // U plane of frame 0; V at + c_plane_stride, frame f at + f * src_frame_stride
    uint8_t *dst;              // [nframes][frame_stride]: the encoder's 4:4:4 layout
    size_t src_frame_stride, c_plane_stride, c_pitch;     // bytes
    size_t frame_stride, plane_stride, row_pitch;
    int w, h, cw, ch, depth, htaps, vtaps;
    const int16_t *hf, *vf;    // [w][UP_TAPS], [h][UP_TAPS]
    const int32_t *hp, *vp;
};

// Where a source's chroma samples are: two planes, or one plane of interleaved pairs (NV12 & co.: U first,
// NV21 & co.: V first).  The kernels below are written once for all three; LAY_PLANAR compiles to what it
// did before the semi-planar front end existed.
enum SrcLayout { LAY_PLANAR = 0, LAY_UV = 1, LAY_VU = 2 };

// the semi-planar front end's extra arguments: src is the interleaved plane (c_plane_stride 0), every sample
// is shifted right by `shift` as it is read (P010: 6); with ysrc the same launch also writes plane 0 from
// that luma (frame f at + f * y_frame_stride, rows y_pitch apart), shifted the same way
struct UpArgsNv : UpArgs {
    const uint8_t *ysrc;
    size_t y_pitch, y_frame_stride;
    int shift;
};

template <int L> struct UpArgsOf { using type = UpArgsNv; };
template <> struct UpArgsOf<LAY_PLANAR> { using type = UpArgs; };

// which interleaved component plane p (1 = U, 2 = V) is
template <int L> __device__ __forceinline__ int comp_of(int p) { return L == LAY_VU ? 2 - p : p - 1; }

template <int L, typename A> __device__ __forceinline__ int shift_of(const A &a)
{
    if constexpr (L == LAY_PLANAR) return 0;
    else return a.shift;
}

// chroma sample i of a row of one plane (planar) or of component `comp` (interleaved)
template <int BPS, int L>
__device__ __forceinline__ int c_sample(const uint8_t *row, int i, int comp, int shift)
{
    if constexpr (L == LAY_PLANAR) {
        return BPS == 1 ? row[i] : reinterpret_cast<const uint16_t *>(row)[i];
    } else {
        const int j = 2 * i + comp;
        return (BPS == 1 ? row[j] : reinterpret_cast<const uint16_t *>(row)[j]) >> shift;
    }
}

template <int BPS, int L = LAY_PLANAR>
__global__ __launch_bounds__(256) void ffv2_upconv_kernel(const typename UpArgsOf<L>::type a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    int p = 1 + (int)(blockIdx.z & 1u), f = (int)(blockIdx.z >> 1);
    if constexpr (L != LAY_PLANAR) {
        if (a.ysrc) {                          // luma blocks in the same grid: z = 3 * frame + plane
            p = (int)(blockIdx.z % 3u); f = (int)(blockIdx.z / 3u);
            if (p == 0) {
                if (x >= a.w) return;
                const uint8_t *row = a.ysrc + (size_t)f * a.y_frame_stride + (size_t)y * a.y_pitch;
                const int v = (BPS == 1 ? row[x] : reinterpret_cast<const uint16_t *>(row)[x]) >> a.shift;
                uint8_t *dp = a.dst + (size_t)f * a.frame_stride + (size_t)y * a.row_pitch;
                if (BPS == 1) dp[x] = (uint8_t)v;
                else reinterpret_cast<uint16_t *>(dp)[x] = (uint16_t)v;
                return;
            }
        }
    }
    if (x >= a.w) return;
    const uint8_t *sp = a.src + (size_t)f * a.src_frame_stride + (size_t)(p - 1) * a.c_plane_stride;
    const int comp = comp_of<L>(p), csh = shift_of<L>(a);
    const int hp = a.hp[x], vp = a.vp[y];
    int hc[UP_TAPS], vc[UP_TAPS];
#pragma unroll
    for (int k = 0; k < UP_TAPS; k++) { hc[k] = a.hf[(size_t)x * UP_TAPS + k]; vc[k] = a.vf[(size_t)y * UP_TAPS + k]; }
    const int hsh = BPS == 1 ? 7 : a.depth - 1;
    const int vsh = BPS == 1 ? 19 : 27 - a.depth;
    int val = BPS == 1 ? 64 << 12 : 1 << (vsh - 1);
    for (int j = 0; j < a.vtaps; j++) {
        const uint8_t *row = sp + (size_t)(vp + j) * a.c_pitch;
        int hv = 0;
        for (int k = 0; k < a.htaps; k++) {
            const int s = c_sample<BPS, L>(row, hp + k, comp, csh);
            hv += s * hc[k];
        }
        hv >>= hsh;
        hv = hv < 32767 ? hv : 32767;
        val += hv * vc[j];
    }
    val >>= vsh;
    const int hi = (1 << a.depth) - 1;
    val = val < 0 ? 0 : (val > hi ? hi : val);
    uint8_t *dp = a.dst + (size_t)f * a.frame_stride + (size_t)p * a.plane_stride + (size_t)y * a.row_pitch;
    if (BPS == 1) dp[x] = (uint8_t)val;
    else reinterpret_cast<uint16_t *>(dp)[x] = (uint16_t)val;
}

// ---- tiled kernel ----
constexpr int UT_W = 128, UT_H = 32;           // output tile
constexpr int UT_SR = 24, UT_SC = 80;          // source patch bound (rows, columns); checked on the host per geometry
constexpr int UT_HP = UT_W + 8;                // int16 per row of the horizontal-pass buffer (272 B rows)

// plane 0 of one output tile from a semi-planar source's luma: 8 samples per item, shifted right by a.shift.
// In place (ysrc = plane 0 of dst, y_pitch = row_pitch) is fine: every item reads the vector it writes.
template <int BPS>
__device__ __forceinline__ void nv_luma_tile(const UpArgsNv &a, int f, int x0, int y0, int t)
{
    const uint8_t *ys = a.ysrc + (size_t)f * a.y_frame_stride;
    uint8_t *yd = a.dst + (size_t)f * a.frame_stride;
#pragma unroll
    for (int it = 0; it < UT_W * UT_H / 8 / 256; it++) {
        const int id = t + 256 * it;
        const int y = y0 + (id >> 4), x = x0 + (id & 15) * 8;
        if (y >= a.h || x >= a.w) continue;
        const uint8_t *sr = ys + (size_t)y * a.y_pitch + (size_t)x * BPS;
        uint32_t v[8];
        if (x + 8 <= a.w && ((uintptr_t)sr & (8 * BPS - 1)) == 0) {
            if constexpr (BPS == 1) {
                const uint2 q = *reinterpret_cast<const uint2 *>(sr);
#pragma unroll
                for (int e = 0; e < 4; e++) { v[e] = (q.x >> (8 * e)) & 0xffu; v[4 + e] = (q.y >> (8 * e)) & 0xffu; }
            } else {
                const uint4 q = *reinterpret_cast<const uint4 *>(sr);
                const uint32_t w[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
                for (int e = 0; e < 4; e++) { v[2 * e] = w[e] & 0xffffu; v[2 * e + 1] = w[e] >> 16; }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++)
                v[e] = x + e < a.w ? (BPS == 1 ? sr[e] : reinterpret_cast<const uint16_t *>(sr)[e]) : 0u;
        }
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] >>= a.shift;
        // the row pitch is a multiple of 128 bytes: a whole vector may be written past the picture's last sample
        uint8_t *dp = yd + (size_t)y * a.row_pitch + (size_t)x * BPS;
        if constexpr (BPS == 1)
            *reinterpret_cast<uint2 *>(dp) = make_uint2(v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24),
                                                        v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24));
        else
            *reinterpret_cast<uint4 *>(dp) = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
    }
}

template <int BPS, int L = LAY_PLANAR>
__global__ __launch_bounds__(256) void ffv2_upconv_tile_kernel(const typename UpArgsOf<L>::type a)
{
    __shared__ uint16_t patch[UT_SR][UT_SC];
    __shared__ __attribute__((aligned(16))) int16_t hbuf[UT_SR][UT_HP];
    __shared__ int16_t vcs[UT_H][4];
    __shared__ int vps[UT_H];
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * UT_W, y0 = blockIdx.y * UT_H;
    int p = 1 + (int)(blockIdx.z & 1u), f = (int)(blockIdx.z >> 1);
    if constexpr (L != LAY_PLANAR) {
        if (a.ysrc) {                          // luma tiles in the same grid: z = 3 * frame + plane
            p = (int)(blockIdx.z % 3u); f = (int)(blockIdx.z / 3u);
            if (p == 0) { nv_luma_tile<BPS>(a, f, x0, y0, t); return; }
        }
    }
    const uint8_t *sp = a.src + (size_t)f * a.src_frame_stride + (size_t)(p - 1) * a.c_plane_stride;
    const int comp = comp_of<L>(p), csh = shift_of<L>(a);
    const int xl = min(x0 + UT_W, a.w) - 1, yl = min(y0 + UT_H, a.h) - 1;     // last output column / row of the tile
    const int cs0 = a.hp[x0], cs1 = min(a.hp[xl] + a.htaps, a.cw);           // source columns [cs0, cs1)
    const int rs0 = a.vp[y0], rs1 = min(a.vp[yl] + a.vtaps, a.ch);
    const int ncols = cs1 - cs0, nrows = rs1 - rs0;
    // source patch -> LDS (rows of <= 80 samples; lanes read consecutive samples)
    for (int i = t; i < nrows * UT_SC; i += 256) {
        const int r = i / UT_SC, c = i - r * UT_SC;
        if (c < ncols) {
            const uint8_t *row = sp + (size_t)(rs0 + r) * a.c_pitch;
            patch[r][c] = (uint16_t)c_sample<BPS, L>(row, cs0 + c, comp, csh);
        }
    }
    if (t < UT_H) {
        const int y = min(y0 + t, a.h - 1);
        vps[t] = a.vp[y] - rs0;
#pragma unroll
        for (int k = 0; k < 4; k++) vcs[t][k] = a.vf[(size_t)y * UP_TAPS + k];
    }
    // this thread's column of the horizontal pass
    const int xc = min(x0 + (t & (UT_W - 1)), a.w - 1);
    const int hp = a.hp[xc] - cs0;
    int hc[4];
#pragma unroll
    for (int k = 0; k < 4; k++) hc[k] = a.hf[(size_t)xc * UP_TAPS + k];
    __syncthreads();
    // horizontal pass: h = min((sum s * c) >> hsh, 32767)   (hScale8To15_c / hScale16To15_c)
    const int hsh = BPS == 1 ? 7 : a.depth - 1;
    for (int r = t >> 7; r < nrows; r += 2) {
        int hv = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = hp + k;
            hv += (k < a.htaps && c < ncols ? (int)patch[r][c] : 0) * hc[k];
        }
        hv >>= hsh;
        hbuf[r][t & (UT_W - 1)] = (int16_t)(hv < 32767 ? hv : 32767);
    }
    __syncthreads();
    // vertical pass: 8 adjacent samples of one row per item   (yuv2planeX_8_c / yuv2planeX_10_c_template)
    const int vsh = BPS == 1 ? 19 : 27 - a.depth;
    const int rnd = BPS == 1 ? 64 << 12 : 1 << (vsh - 1);
    const int hi = (1 << a.depth) - 1;
#pragma unroll
    for (int it = 0; it < UT_W * UT_H / 8 / 256; it++) {
        const int id = t + 256 * it;
        const int ty = id >> 4, xg = (id & 15) * 8;
        const int y = y0 + ty, x = x0 + xg;
        if (y >= a.h || x >= a.w) continue;
        int acc[8];
#pragma unroll
        for (int e = 0; e < 8; e++) acc[e] = rnd;
        const int vp = vps[ty];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = vp + j;
            const int c = vcs[ty][j];
            if (j < a.vtaps && r < nrows) {
                const int4 w = *reinterpret_cast<const int4 *>(&hbuf[r][xg]);
                const int wv[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    acc[2 * q]     += ((wv[q] << 16) >> 16) * c;
                    acc[2 * q + 1] += (wv[q] >> 16) * c;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int v = acc[e] >> vsh;
            acc[e] = v < 0 ? 0 : (v > hi ? hi : v);
        }
        // the row pitch is a multiple of 128 bytes: a whole vector may be written where the picture
        // ends inside it (the padding behind the last sample is never read as picture)
        uint8_t *dp = a.dst + (size_t)f * a.frame_stride + (size_t)p * a.plane_stride + (size_t)y * a.row_pitch;
        if (BPS == 1) {
            const uint2 o = make_uint2((uint32_t)acc[0] | ((uint32_t)acc[1] << 8) | ((uint32_t)acc[2] << 16) | ((uint32_t)acc[3] << 24),
                                       (uint32_t)acc[4] | ((uint32_t)acc[5] << 8) | ((uint32_t)acc[6] << 16) | ((uint32_t)acc[7] << 24));
            *reinterpret_cast<uint2 *>(dp + x) = o;
        } else {
            const uint4 o = make_uint4((uint32_t)acc[0] | ((uint32_t)acc[1] << 16), (uint32_t)acc[2] | ((uint32_t)acc[3] << 16),
                                       (uint32_t)acc[4] | ((uint32_t)acc[5] << 16), (uint32_t)acc[6] | ((uint32_t)acc[7] << 16));
            *reinterpret_cast<uint4 *>(dp + (size_t)x * 2) = o;
        }
    }
}

}  // namespace

struct FFV2Upconv {
    int w = 0, h = 0, depth = 0, htaps = 0, vtaps = 0;
    bool tiled = false;        // every 128 x 32 output tile's source patch fits the tiled kernel's LDS
    int16_t *d_hf = nullptr, *d_vf = nullptr;
    int32_t *d_hp = nullptr, *d_vp = nullptr;
};

void ffv2_upconv_destroy(FFV2Upconv *u)
{
    if (!u) return;
    (void)hipFree(u->d_hf); (void)hipFree(u->d_vf); (void)hipFree(u->d_hp); (void)hipFree(u->d_vp);
    delete u;
}

// coefficient tables for a w x h picture of `depth` bits; nullptr if the geometry has no
// 4-tap-or-less... i.e. no table that fits (never for pictures of 8 x 8 and more)
FFV2Upconv *ffv2_upconv_create(int w, int h, int depth)
{
    AxisFilter hx, vy;
    try {
        if (!build_axis(hx, w, 1 << 14) || !build_axis(vy, h, 1 << 12)) return nullptr;   // :1681,:1714
    } catch (...) { return nullptr; }
    FFV2Upconv *u = new (std::nothrow) FFV2Upconv;
    if (!u) return nullptr;
    u->w = w; u->h = h; u->depth = depth; u->htaps = hx.taps; u->vtaps = vy.taps;
    {
        const int cw = (w + 1) >> 1, ch = (h + 1) >> 1;
        bool fits = hx.taps <= 4 && vy.taps <= 4;
        for (int x0 = 0; x0 < w && fits; x0 += UT_W) {
            const int xl = (x0 + UT_W < w ? x0 + UT_W : w) - 1;
            int c1 = hx.pos[(size_t)xl] + hx.taps;
            if (c1 > cw) c1 = cw;
            fits = c1 - hx.pos[(size_t)x0] <= UT_SC && hx.pos[(size_t)x0] >= 0;
            for (int x = x0; x <= xl && fits; x++) fits = hx.pos[(size_t)x] >= hx.pos[(size_t)x0] && hx.pos[(size_t)x] <= hx.pos[(size_t)xl];
        }
        for (int y0 = 0; y0 < h && fits; y0 += UT_H) {
            const int yl = (y0 + UT_H < h ? y0 + UT_H : h) - 1;
            int r1 = vy.pos[(size_t)yl] + vy.taps;
            if (r1 > ch) r1 = ch;
            fits = r1 - vy.pos[(size_t)y0] <= UT_SR && vy.pos[(size_t)y0] >= 0;
            for (int y = y0; y <= yl && fits; y++) fits = vy.pos[(size_t)y] >= vy.pos[(size_t)y0] && vy.pos[(size_t)y] <= vy.pos[(size_t)yl];
        }
        u->tiled = fits;
    }
    bool ok = hipMalloc(&u->d_hf, hx.coef.size() * 2) == hipSuccess && hipMalloc(&u->d_vf, vy.coef.size() * 2) == hipSuccess &&
              hipMalloc(&u->d_hp, hx.pos.size() * 4) == hipSuccess && hipMalloc(&u->d_vp, vy.pos.size() * 4) == hipSuccess;
    ok = ok && hipMemcpy(u->d_hf, hx.coef.data(), hx.coef.size() * 2, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(u->d_vf, vy.coef.data(), vy.coef.size() * 2, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(u->d_hp, hx.pos.data(), hx.pos.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(u->d_vp, vy.pos.data(), vy.pos.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipStreamSynchronize(nullptr) == hipSuccess;      // null stream: the callers' streams do not wait for it
    if (!ok) { ffv2_upconv_destroy(u); return nullptr; }
    return u;
}

size_t ffv2_upconv_src_frame_bytes(int w, int h, int depth)
{
    const size_t bps = depth > 8 ? 2 : 1;
    return ((size_t)w * h + 2 * (size_t)((w + 1) >> 1) * ((h + 1) >> 1)) * bps;
}

// chroma planes only: src_u = U plane of frame 0 (rows c_pitch bytes apart), V at + c_plane_stride,
// the next frame at + src_frame_stride; dst = the encoder's 4:4:4 frames (planes 1 and 2 are written)
hipError_t ffv2_launch_upconv_chroma(const FFV2Upconv *u, const FFV2Geom &g, int nframes, const uint8_t *src_u,
                                     size_t c_pitch, size_t c_plane_stride, size_t src_frame_stride, uint8_t *dst,
                                     hipStream_t s)
{
    const int bps = g.bytes_per_sample;
    UpArgs a{};
    a.src = src_u; a.dst = dst; a.src_frame_stride = src_frame_stride; a.c_plane_stride = c_plane_stride; a.c_pitch = c_pitch;
    a.frame_stride = g.frame_stride; a.plane_stride = g.plane_stride; a.row_pitch = g.row_pitch;
    a.w = g.width; a.h = g.height; a.cw = (g.width + 1) >> 1; a.ch = (g.height + 1) >> 1; a.depth = g.depth;
    a.htaps = u->htaps; a.vtaps = u->vtaps; a.hf = u->d_hf; a.vf = u->d_vf; a.hp = u->d_hp; a.vp = u->d_vp;
    static const int force_naive = getenv("FFV2AMD_UPCONV_NAIVE") ? atoi(getenv("FFV2AMD_UPCONV_NAIVE")) : 0;
    if (u->tiled && !force_naive) {
        const dim3 grid((unsigned)((g.width + UT_W - 1) / UT_W), (unsigned)((g.height + UT_H - 1) / UT_H), (unsigned)(2 * nframes)), block(256);
        if (bps == 1) hipLaunchKernelGGL(ffv2_upconv_tile_kernel<1>, grid, block, 0, s, a);
        else          hipLaunchKernelGGL(ffv2_upconv_tile_kernel<2>, grid, block, 0, s, a);
    } else {
        const dim3 grid((unsigned)((g.width + 255) / 256), (unsigned)g.height, (unsigned)(2 * nframes)), block(256);
        if (bps == 1) hipLaunchKernelGGL(ffv2_upconv_kernel<1>, grid, block, 0, s, a);
        else          hipLaunchKernelGGL(ffv2_upconv_kernel<2>, grid, block, 0, s, a);
    }
    return hipGetLastError();
}

// tightly packed 4:2:0 frames (Y, U, V back to back) -> 4:4:4 frames
hipError_t ffv2_launch_upconv(const FFV2Upconv *u, const FFV2Geom &g, int nframes, const uint8_t *src,
                              size_t src_frame_stride, uint8_t *dst, hipStream_t s)
{
    const int bps = g.bytes_per_sample;
    // luma: the identity -- rows copied into the encoder's pitched layout
    for (int f = 0; f < nframes; f++) {
        const hipError_t rc = hipMemcpy2DAsync(dst + (size_t)f * g.frame_stride, g.row_pitch, src + (size_t)f * src_frame_stride,
                                               (size_t)g.width * bps, (size_t)g.width * bps, (size_t)g.height,
                                               hipMemcpyDeviceToDevice, s);
        if (rc != hipSuccess) return rc;
    }
    const size_t cw = (size_t)((g.width + 1) >> 1), ch = (size_t)((g.height + 1) >> 1);
    return ffv2_launch_upconv_chroma(u, g, nframes, src + (size_t)g.width * g.height * bps, cw * bps, cw * ch * bps,
                                     src_frame_stride, dst, s);
}

// =============================================================================================
// 4:2:2 -> 4:4:4.  For a yuv422p / yuv422p10le / yuv422p12le source the tool chain does the same
// thing as for 4:2:0 with one axis less:
//   format   av_find_best_pix_fmt_of_2 / get_pix_fmt_score (libavutil/pixdesc.c:2838-2873) pick
//            yuv444p* of the same depth (no loss; ties go to the smaller format);
//   scaler   ff_get_unscaled_swscale has no converter for the pair, the subsampling differs
//            (swscale_unscaled.c:2122-2137): the generic scaler runs;
//   chroma x vf_scale's default chroma position -513 (the YUV420P override, vf_scale.c:566-572,
//            does not apply) becomes 128 on a subsampled axis (get_local_pos, utils.c:303-310): the
//            horizontal filter is the 4:2:0 one, build_axis(w, 1 << 14) over ceil(w/2) samples;
//            h = min((sum s * hf) >> (8-bit: 7 | deeper: depth-1), 32767)   (swscale.c:96-139)
//   chroma y not subsampled: src pos = dst pos = 128, chrYInc = 1 << 16, so initFilter's unscaled
//            branch (utils.c:353-362) gives filter size 1 and vscale.c:274,90-91 calls yuv2plane1:
//              8 bit:  out = clip_u8((h + 64) >> 7)   (constant dither 64: 8-bit sources are not
//                      dithered, swscale.c:263,346; output.c:395-403)
//              deeper: out = clip((h + (1 << (14-d))) >> (15-d), 0, 2^d - 1)   (output.c:320-330)
//   luma     the identity.
// Because initFilter normalises every vertical row to exactly 4096, the 4:2:0 path fed chroma that
// is constant along y gives this result in every row -- the tests tie the two together that way.
// PARITY UNPINNED, as for 4:2:0: no libswscale binary or vector exists here.
//
// Device part: every output row depends on one source row, so there is no LDS transpose and no
// vertical pass: ffv2_upconv422_kernel is a streaming 2x horizontal bicubic.  A wave owns a
// 64 * (16 / bytes per sample) wide strip of one row at a time: its source span (coalesced loads)
// goes to LDS, each lane then writes one 16-byte vector of consecutive output samples from its
// 4 taps per sample; the lane's positions and coefficients stay in registers for the 4 rows the
// wave does.  ffv2_upconv422_naive_kernel (one thread per sample, any tap count) is the fallback
// for tables the strip does not fit -- none that build_axis makes for w >= 12 -- and can be forced
// with FFV2AMD_UPCONV422_NAIVE=1 (read per launch).
// =============================================================================================
namespace {

template <int BPS> struct U2Shape {
    static constexpr int VEC = 16 / BPS;       // output samples per lane: one 16-byte store
    static constexpr int TW = 64 * VEC;        // output columns per strip
    static constexpr int SPAN = TW / 2 + 32;   // source samples a strip may read (checked on the host)
    static constexpr int LOADS = (SPAN + 63) / 64;   // loads per lane and source row
    static constexpr int RW = BPS == 2 ? 8 : 4;      // rows per wave: all their loads are in flight at once
    static constexpr int ROWS = 4 * RW;              // output rows per workgroup
};

struct Up422Args {
    const uint8_t *src;        // U plane of frame 0; V at + c_plane_stride, frame f at + f * src_frame_stride
    uint8_t *dst;              // [nframes][frame_stride]: the encoder's 4:4:4 layout
    size_t src_frame_stride, c_plane_stride, c_pitch;     // bytes
    size_t frame_stride, plane_stride, row_pitch;
    int w, h, cw, depth, htaps;
    const int16_t *hf;         // [w][UP_TAPS], zero beyond htaps
    const int32_t *hp;         // [w]
};

// the vertical no-op of yuv2plane1: 15-bit intermediate -> output sample.  The intermediate is an int16_t in
// swscale (hScale*To15's dst): a sum below -32768, which only samples above the depth reach, wraps.
template <int BPS>
__device__ __forceinline__ int u2_out(int hv, int depth)
{
    hv = (int16_t)(hv < 32767 ? hv : 32767);
    const int v = BPS == 1 ? (hv + 64) >> 7 : (hv + (1 << (14 - depth))) >> (15 - depth);
    const int hi = (1 << depth) - 1;
    return v < 0 ? 0 : (v > hi ? hi : v);
}

// interleaved (NV16) sources: src is the UV plane (c_plane_stride 0), component by comp_of<L>, no shift
template <int BPS, int L = LAY_PLANAR>
__global__ __launch_bounds__(256) void ffv2_upconv422_kernel(const Up422Args a)
{
    using S = U2Shape<BPS>;
    constexpr int VEC = S::VEC, TW = S::TW, SPAN = S::SPAN, RW = S::RW;
    constexpr int PAIR = L == LAY_PLANAR ? 1 : 2;       // samples per source column
    __shared__ uint16_t span[4][RW][SPAN];     // [wave][row]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = blockIdx.x * TW, yw = blockIdx.y * S::ROWS + wv * RW;    // the wave's rows: yw .. yw + RW - 1
    const int p = 1 + (int)(blockIdx.z & 1u), f = (int)(blockIdx.z >> 1);
    const int comp = comp_of<L>(p);
    const int xl = min(x0 + TW, a.w) - 1;
    const int s0 = a.hp[x0], ns = min(a.hp[xl] + a.htaps, a.cw) - s0;      // source columns [s0, s0 + ns)
    const uint8_t *sp = a.src + (size_t)f * a.src_frame_stride + (size_t)(p - 1) * a.c_plane_stride + (size_t)s0 * BPS * PAIR;
    // the source spans of the wave's rows -> LDS, four rows at a time: the loads are unconditional (indices clamped
    // into the span and the picture) so that all of them are in flight before the first is waited for
#pragma unroll
    for (int j0 = 0; j0 < RW; j0 += 4) {
        uint32_t v[4][S::LOADS];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint8_t *row = sp + (size_t)min(yw + j0 + j, a.h - 1) * a.c_pitch;
#pragma unroll
            for (int k = 0; k < S::LOADS; k++) {
                const int i = min(lane + 64 * k, ns - 1);
                v[j][k] = (uint32_t)c_sample<BPS, L>(row, i, comp, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < S::LOADS; k++)
                if (lane + 64 * k < ns) span[wv][j0 + j][lane + 64 * k] = (uint16_t)v[j][k];
    }
    // this lane's VEC outputs: positions relative to s0, 4 coefficients each (zero beyond htaps)
    const int x = x0 + lane * VEC;
    int pos[VEC];
    uint2 cf[VEC];
#pragma unroll
    for (int e = 0; e < VEC; e++) {
        const int xe = min(x + e, xl);
        pos[e] = a.hp[xe] - s0;
        cf[e] = *reinterpret_cast<const uint2 *>(a.hf + (size_t)xe * UP_TAPS);
    }
    __syncthreads();
    if (x >= a.w) return;
    const int hsh = BPS == 1 ? 7 : a.depth - 1;
    uint8_t *dp = a.dst + (size_t)f * a.frame_stride + (size_t)p * a.plane_stride + (size_t)x * BPS;
#pragma unroll 2
    for (int j = 0; j < RW; j++) {
        const int y = yw + j;
        if (y >= a.h) break;
        int o[VEC];
#pragma unroll
        for (int e = 0; e < VEC; e++) {
            const uint16_t *s = &span[wv][j][pos[e]];
            const int hv = (int)s[0] * ((int)(cf[e].x << 16) >> 16) + (int)s[1] * ((int)cf[e].x >> 16) +
                           (int)s[2] * ((int)(cf[e].y << 16) >> 16) + (int)s[3] * ((int)cf[e].y >> 16);
            o[e] = u2_out<BPS>(hv >> hsh, a.depth);
        }
        // the row pitch is a multiple of 128 bytes: a whole vector may be written where the picture
        // ends inside it (the padding behind the last sample is never read as picture)
        uint4 v;
        if constexpr (BPS == 1) {
            v = make_uint4((uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24),
                           (uint32_t)o[4] | ((uint32_t)o[5] << 8) | ((uint32_t)o[6] << 16) | ((uint32_t)o[7] << 24),
                           (uint32_t)o[8] | ((uint32_t)o[9] << 8) | ((uint32_t)o[10] << 16) | ((uint32_t)o[11] << 24),
                           (uint32_t)o[12] | ((uint32_t)o[13] << 8) | ((uint32_t)o[14] << 16) | ((uint32_t)o[15] << 24));
        } else {
            v = make_uint4((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16),
                           (uint32_t)o[4] | ((uint32_t)o[5] << 16), (uint32_t)o[6] | ((uint32_t)o[7] << 16));
        }
        *reinterpret_cast<uint4 *>(dp + (size_t)y * a.row_pitch) = v;
    }
}

// one thread per output sample, any tap count up to UP_TAPS, taps read from global memory
template <int BPS, int L = LAY_PLANAR>
__global__ __launch_bounds__(256) void ffv2_upconv422_naive_kernel(const Up422Args a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const int p = 1 + (int)(blockIdx.z & 1u), f = (int)(blockIdx.z >> 1);
    if (x >= a.w) return;
    const uint8_t *row = a.src + (size_t)f * a.src_frame_stride + (size_t)(p - 1) * a.c_plane_stride + (size_t)y * a.c_pitch;
    const int hp = a.hp[x];
    int hv = 0;
    for (int k = 0; k < a.htaps; k++) {
        const int s = c_sample<BPS, L>(row, hp + k, comp_of<L>(p), 0);
        hv += s * a.hf[(size_t)x * UP_TAPS + k];
    }
    const int v = u2_out<BPS>(hv >> (BPS == 1 ? 7 : a.depth - 1), a.depth);
    uint8_t *dp = a.dst + (size_t)f * a.frame_stride + (size_t)p * a.plane_stride + (size_t)y * a.row_pitch;
    if (BPS == 1) dp[x] = (uint8_t)v;
    else reinterpret_cast<uint16_t *>(dp)[x] = (uint16_t)v;
}

}  // namespace

struct FFV2Upconv422 {
    int w = 0, depth = 0, htaps = 0;
    bool strips = false;       // every strip's source span fits ffv2_upconv422_kernel's LDS
    int16_t *d_hf = nullptr;
    int32_t *d_hp = nullptr;
};

void ffv2_upconv422_destroy(FFV2Upconv422 *u)
{
    if (!u) return;
    (void)hipFree(u->d_hf); (void)hipFree(u->d_hp);
    delete u;
}

// the horizontal table of a w-wide picture (any height); nullptr where that axis does not build --
// the horizontal half of ffv2_upconv_create's rule.  Uploaded on `s`, which is waited for.
FFV2Upconv422 *ffv2_upconv422_create(int w, int depth, hipStream_t s)
{
    AxisFilter hx;
    try {
        if (!build_axis(hx, w, 1 << 14)) return nullptr;                     // :1681
    } catch (...) { return nullptr; }
    FFV2Upconv422 *u = new (std::nothrow) FFV2Upconv422;
    if (!u) return nullptr;
    u->w = w; u->depth = depth; u->htaps = hx.taps;
    {
        const int cw = (w + 1) >> 1;
        const int tw = depth > 8 ? U2Shape<2>::TW : U2Shape<1>::TW, span = depth > 8 ? U2Shape<2>::SPAN : U2Shape<1>::SPAN;
        bool fits = hx.taps <= 4;
        for (int x0 = 0; x0 < w && fits; x0 += tw) {
            const int xl = (x0 + tw < w ? x0 + tw : w) - 1;
            int c1 = hx.pos[(size_t)xl] + hx.taps;
            if (c1 > cw) c1 = cw;
            // the strip's span plus the 4-tap reads of its last sample stay inside the LDS row
            fits = hx.pos[(size_t)x0] >= 0 && c1 - hx.pos[(size_t)x0] + 4 <= span &&
                   hx.pos[(size_t)xl] - hx.pos[(size_t)x0] + 4 <= span;
            for (int x = x0; x <= xl && fits; x++) fits = hx.pos[(size_t)x] >= hx.pos[(size_t)x0] && hx.pos[(size_t)x] <= hx.pos[(size_t)xl];
        }
        u->strips = fits;
    }
    bool ok = hipMalloc(&u->d_hf, hx.coef.size() * 2) == hipSuccess && hipMalloc(&u->d_hp, hx.pos.size() * 4) == hipSuccess;
    ok = ok && hipMemcpyAsync(u->d_hf, hx.coef.data(), hx.coef.size() * 2, hipMemcpyHostToDevice, s) == hipSuccess &&
         hipMemcpyAsync(u->d_hp, hx.pos.data(), hx.pos.size() * 4, hipMemcpyHostToDevice, s) == hipSuccess &&
         hipStreamSynchronize(s) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); ffv2_upconv422_destroy(u); return nullptr; }
    return u;
}

size_t ffv2_upconv422_src_frame_bytes(int w, int h, int depth)
{
    const size_t bps = depth > 8 ? 2 : 1;
    return ((size_t)w * h + 2 * (size_t)((w + 1) >> 1) * h) * bps;
}

bool ffv2_upconv422_uses_strips(const FFV2Upconv422 *u)
{
    const char *force = getenv("FFV2AMD_UPCONV422_NAIVE");
    return u->strips && !(force && atoi(force));
}

// chroma planes only: src_u = U plane of frame 0 (h rows, c_pitch bytes apart), V at + c_plane_stride, the
// next frame at + src_frame_stride; dst = the encoder's 4:4:4 frames (planes 1 and 2 are written)
hipError_t ffv2_launch_upconv422_chroma(const FFV2Upconv422 *u, const FFV2Geom &g, int nframes, const uint8_t *src_u,
                                        size_t c_pitch, size_t c_plane_stride, size_t src_frame_stride, uint8_t *dst,
                                        hipStream_t s)
{
    const int bps = g.bytes_per_sample;
    Up422Args a{};
    a.src = src_u; a.dst = dst; a.src_frame_stride = src_frame_stride; a.c_plane_stride = c_plane_stride; a.c_pitch = c_pitch;
    a.frame_stride = g.frame_stride; a.plane_stride = g.plane_stride; a.row_pitch = g.row_pitch;
    a.w = g.width; a.h = g.height; a.cw = (g.width + 1) >> 1; a.depth = g.depth;
    a.htaps = u->htaps; a.hf = u->d_hf; a.hp = u->d_hp;
    if (ffv2_upconv422_uses_strips(u)) {
        const int tw = bps == 1 ? U2Shape<1>::TW : U2Shape<2>::TW;
        const int rows = bps == 1 ? U2Shape<1>::ROWS : U2Shape<2>::ROWS;
        const dim3 grid((unsigned)((g.width + tw - 1) / tw), (unsigned)((g.height + rows - 1) / rows), (unsigned)(2 * nframes)), block(256);
        if (bps == 1) hipLaunchKernelGGL(ffv2_upconv422_kernel<1>, grid, block, 0, s, a);
        else          hipLaunchKernelGGL(ffv2_upconv422_kernel<2>, grid, block, 0, s, a);
    } else {
        const dim3 grid((unsigned)((g.width + 255) / 256), (unsigned)g.height, (unsigned)(2 * nframes)), block(256);
        if (bps == 1) hipLaunchKernelGGL(ffv2_upconv422_naive_kernel<1>, grid, block, 0, s, a);
        else          hipLaunchKernelGGL(ffv2_upconv422_naive_kernel<2>, grid, block, 0, s, a);
    }
    return hipGetLastError();
}

// tightly packed 4:2:2 frames (Y, U, V back to back) -> 4:4:4 frames
hipError_t ffv2_launch_upconv422(const FFV2Upconv422 *u, const FFV2Geom &g, int nframes, const uint8_t *src,
                                 size_t src_frame_stride, uint8_t *dst, hipStream_t s)
{
    const int bps = g.bytes_per_sample;
    for (int f = 0; f < nframes; f++) {       // luma: the identity
        const hipError_t rc = hipMemcpy2DAsync(dst + (size_t)f * g.frame_stride, g.row_pitch, src + (size_t)f * src_frame_stride,
                                               (size_t)g.width * bps, (size_t)g.width * bps, (size_t)g.height,
                                               hipMemcpyDeviceToDevice, s);
        if (rc != hipSuccess) return rc;
    }
    const size_t cw = (size_t)((g.width + 1) >> 1);
    return ffv2_launch_upconv422_chroma(u, g, nframes, src + (size_t)g.width * g.height * bps, cw * bps, cw * g.height * bps,
                                        src_frame_stride, dst, s);
}

// =============================================================================================
// Semi-planar sources: one plane of interleaved chroma pairs instead of two planes.
//   nv12 / nv21 / p010le   4:2:0, 8 / 8 / 10 bit;  nv16  4:2:2, 8 bit;  nv24 / nv42  4:4:4, 8 bit.
// What the reference tool chain makes of them before encode2() (ffv2enc.c:596-601 lists yuv444p* only):
//   format   av_find_best_pix_fmt_of_2 / get_pix_fmt_score (libavutil/pixdesc.c:2838-2873) picks the
//            yuv444p* format of the same component depth: the loss flags of a deeper or a subsampled
//            candidate cost more, and P010's depth is 10 (pixdesc.c:2102-2113), so yuv444p10le;
//   input    libswscale's input readers only de-interleave (nvXXtoUV_c, libswscale/input.c:686-698);
//            P010's also shift every sample right by 6, dropping the low 6 bits (p010LEToY_c /
//            p010LEToUV_c, input.c:700-726), and the scaler then runs at c->srcBpc = 10
//            (libswscale/utils.c:1416-1418);
//   4:2:0 / 4:2:2  the generic scaler follows on those planes exactly as for yuv420p* / yuv422p*: the
//            4:2:0 and 4:2:2 paths above, reading the interleaved plane (ffv2_upconv_tile_kernel /
//            ffv2_upconv_kernel / ffv2_upconv422_kernel / ffv2_upconv422_naive_kernel with L = LAY_UV,
//            LAY_VU);
//   4:4:4    ff_get_unscaled_swscale has an exact converter for nv24 / nv42 -> yuv444p
//            (nv24ToPlanarWrapper, libswscale/swscale_unscaled.c:1926-1930): a pure de-interleave,
//            ffv2_nv444_kernel.
// PARITY UNPINNED, as for the planar front ends: no libswscale binary or vector exists here.
//
// Device part: sources are pitched (decoder surfaces are padded): luma pitch, chroma pitch and frame
// stride are separate.  A 4:2:0 / 4:2:2 workgroup reads its component of the pairs straight from
// the interleaved rows (every other sample).  P010 luma needs the shift, so the 4:2:0 launch carries
// luma tiles in the same grid (z = 3 * frame + plane) -- also in place, where the ring's DMA has put
// the raw samples into plane 0 already; 8-bit luma is a plain copy (DMA).
// =============================================================================================
namespace {

struct Nv444Args {
    const uint8_t *uv;         // frame 0's interleaved plane, rows uv_pitch apart, frame f at + f * src_frame_stride
    size_t uv_pitch, src_frame_stride;
    uint8_t *dst;
    size_t frame_stride, plane_stride, row_pitch;
    int w, h;
};

// 8-bit nv24 / nv42 -> planes 1 and 2: a lane takes 8 pairs (one 16-byte load where the row allows it)
// and writes 8 samples to each plane; a wave takes 512 columns of one row, a workgroup 4 rows
template <int L>
__global__ __launch_bounds__(256) void ffv2_nv444_kernel(const Nv444Args a)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = (blockIdx.x * 64 + lane) * 8, y = blockIdx.y * 4 + wv, f = blockIdx.z;
    if (x >= a.w || y >= a.h) return;
    const uint8_t *s = a.uv + (size_t)f * a.src_frame_stride + (size_t)y * a.uv_pitch + (size_t)x * 2;
    uint32_t w[4];
    if (x + 8 <= a.w && ((uintptr_t)s & 15) == 0) {
        const uint4 q = *reinterpret_cast<const uint4 *>(s);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            w[i] = 0;
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (x + 2 * i + (b >> 1) < a.w) w[i] |= (uint32_t)s[4 * i + b] << (8 * b);
        }
    }
    // bytes 0, 2 of each dword are the first component, 1, 3 the second (v_perm_b32 material)
    const uint32_t c0lo = (w[0] & 0xffu) | ((w[0] >> 8) & 0xff00u) | ((w[1] << 16) & 0xff0000u) | ((w[1] << 8) & 0xff000000u);
    const uint32_t c0hi = (w[2] & 0xffu) | ((w[2] >> 8) & 0xff00u) | ((w[3] << 16) & 0xff0000u) | ((w[3] << 8) & 0xff000000u);
    const uint32_t c1lo = ((w[0] >> 8) & 0xffu) | ((w[0] >> 16) & 0xff00u) | ((w[1] << 8) & 0xff0000u) | (w[1] & 0xff000000u);
    const uint32_t c1hi = ((w[2] >> 8) & 0xffu) | ((w[2] >> 16) & 0xff00u) | ((w[3] << 8) & 0xff0000u) | (w[3] & 0xff000000u);
    // the row pitch is a multiple of 128 bytes: the 8 samples may run past the picture's last one
    uint8_t *d = a.dst + (size_t)f * a.frame_stride + (size_t)y * a.row_pitch + x;
    uint8_t *du = d + a.plane_stride, *dv = d + 2 * a.plane_stride;
    *reinterpret_cast<uint2 *>(L == LAY_VU ? dv : du) = make_uint2(c0lo, c0hi);
    *reinterpret_cast<uint2 *>(L == LAY_VU ? du : dv) = make_uint2(c1lo, c1hi);
}

}  // namespace

hipError_t ffv2_launch_nv420(const FFV2Upconv *u, const FFV2Geom &g, int nframes, const FFV2NvSrc &src, uint8_t *dst,
                             hipStream_t s)
{
    const int bps = g.bytes_per_sample;
    UpArgsNv a{};
    a.src = src.uv; a.dst = dst; a.src_frame_stride = src.frame_stride; a.c_plane_stride = 0; a.c_pitch = src.uv_pitch;
    a.frame_stride = g.frame_stride; a.plane_stride = g.plane_stride; a.row_pitch = g.row_pitch;
    a.w = g.width; a.h = g.height; a.cw = (g.width + 1) >> 1; a.ch = (g.height + 1) >> 1; a.depth = g.depth;
    a.htaps = u->htaps; a.vtaps = u->vtaps; a.hf = u->d_hf; a.vf = u->d_vf; a.hp = u->d_hp; a.vp = u->d_vp;
    a.ysrc = src.y; a.y_pitch = src.y_pitch; a.y_frame_stride = src.y_frame_stride; a.shift = src.shift;
    const unsigned nz = (unsigned)((src.y ? 3 : 2) * nframes);
    static const int force_naive = getenv("FFV2AMD_UPCONV_NAIVE") ? atoi(getenv("FFV2AMD_UPCONV_NAIVE")) : 0;
#define NV_LAUNCH(K, grid)                                                                                      \
    do {                                                                                                        \
        if (bps == 1 && !src.vu) hipLaunchKernelGGL((K<1, LAY_UV>), grid, dim3(256), 0, s, a);                  \
        else if (bps == 1)       hipLaunchKernelGGL((K<1, LAY_VU>), grid, dim3(256), 0, s, a);                  \
        else                     hipLaunchKernelGGL((K<2, LAY_UV>), grid, dim3(256), 0, s, a);                  \
    } while (0)
    if (bps == 2 && src.vu) return hipErrorInvalidValue;       // no 16-bit V-first 4:2:0 source is accepted
    if (u->tiled && !force_naive)
        NV_LAUNCH(ffv2_upconv_tile_kernel, dim3((unsigned)((g.width + UT_W - 1) / UT_W), (unsigned)((g.height + UT_H - 1) / UT_H), nz));
    else
        NV_LAUNCH(ffv2_upconv_kernel, dim3((unsigned)((g.width + 255) / 256), (unsigned)g.height, nz));
#undef NV_LAUNCH
    return hipGetLastError();
}

hipError_t ffv2_launch_nv422(const FFV2Upconv422 *u, const FFV2Geom &g, int nframes, const FFV2NvSrc &src, uint8_t *dst,
                             hipStream_t s)
{
    if (g.bytes_per_sample != 1 || src.vu || src.y || src.shift) return hipErrorInvalidValue;     // nv16 only
    Up422Args a{};
    a.src = src.uv; a.dst = dst; a.src_frame_stride = src.frame_stride; a.c_plane_stride = 0; a.c_pitch = src.uv_pitch;
    a.frame_stride = g.frame_stride; a.plane_stride = g.plane_stride; a.row_pitch = g.row_pitch;
    a.w = g.width; a.h = g.height; a.cw = (g.width + 1) >> 1; a.depth = g.depth;
    a.htaps = u->htaps; a.hf = u->d_hf; a.hp = u->d_hp;
    if (ffv2_upconv422_uses_strips(u)) {
        const dim3 grid((unsigned)((g.width + U2Shape<1>::TW - 1) / U2Shape<1>::TW),
                        (unsigned)((g.height + U2Shape<1>::ROWS - 1) / U2Shape<1>::ROWS), (unsigned)(2 * nframes));
        hipLaunchKernelGGL((ffv2_upconv422_kernel<1, LAY_UV>), grid, dim3(256), 0, s, a);
    } else {
        const dim3 grid((unsigned)((g.width + 255) / 256), (unsigned)g.height, (unsigned)(2 * nframes));
        hipLaunchKernelGGL((ffv2_upconv422_naive_kernel<1, LAY_UV>), grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t ffv2_launch_nv444(const FFV2Geom &g, int nframes, const FFV2NvSrc &src, uint8_t *dst, hipStream_t s)
{
    if (g.bytes_per_sample != 1 || src.y || src.shift) return hipErrorInvalidValue;               // nv24 / nv42 only
    Nv444Args a{};
    a.uv = src.uv; a.uv_pitch = src.uv_pitch; a.src_frame_stride = src.frame_stride; a.dst = dst;
    a.frame_stride = g.frame_stride; a.plane_stride = g.plane_stride; a.row_pitch = g.row_pitch;
    a.w = g.width; a.h = g.height;
    const dim3 grid((unsigned)((g.width + 511) / 512), (unsigned)((g.height + 3) / 4), (unsigned)nframes), block(256);
    if (src.vu) hipLaunchKernelGGL(ffv2_nv444_kernel<LAY_VU>, grid, block, 0, s, a);
    else        hipLaunchKernelGGL(ffv2_nv444_kernel<LAY_UV>, grid, block, 0, s, a);
    return hipGetLastError();
}
