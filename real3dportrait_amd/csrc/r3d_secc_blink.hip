// Blink edit of SECC maps: blink_eye_for_secc of inference/edit_secc.py:47-129 for the F selected frames of a clip in one chain of launches,
// without the reference's host round trip and its two sklearn kd-trees (tests/blink_ref.py is the NumPy restatement).
// For one map img [3, h, w] in [-1, 1] and p = close_eye_percent:
//   quantise   q = trunc(((img + 1) / 2) 255) per channel, each operation rounded to fp32; NaN and values outside [-1, 1] clamp to 0 .. 255
//              (the reference's astype(np.uint) is undefined there).  out = q / 127.5 - 1 (IEEE division, then the subtraction).  p == 0 ends here.
//   face       all three q non-zero.  L = rows [h/4, h/2) x cols [w/4, w/2), R = the same rows x cols [w/2, 3 (w/4)) (integer divisions).
//   E          ~face & (L | R); min_h, max_h over E's rows; lmin, lmax over the columns of ~face & L; rmin, rmax over those of ~face & R.
//   P          rows [min_h - 4, max_h + 4) x (cols [lmin - 4, lmax + 4) u cols [rmin - 4, rmax + 4)), ends exclusive, clamped to the image.
//   F          face & P without every pixel that has a pixel of E (all of E, not E & P) at d^2 <= 25;  M = ~F & P.
//   columns    per column over M: cnt, sum and min / max of the row indices; mean = sum / max(cnt, 1), lo = p mean + (1 - p) min,
//              hi = p mean + (1 - p) max in fp64, every operation rounded on its own (contraction off: no fused multiply-add);
//              B = the pixels of M with row <= lo or row >= hi.
//   fill       every pixel of B takes the q of its nearest pixel of F, the minimum of the key (d^2, row, col): on a distance tie the lowest
//              (row, col), where the reference takes whatever its kd-tree returns.  A pure function of the input.
//   status     0 done; 1 no eye pixel in L or in R, 2 F empty (the reference raises ValueError): the map is quantised only;
//              3 frame index outside [0, T) or p outside [0, 1] (NaN too): the frame is not read and not written.
// Four kernels behind one async memset of the per-frame heads (bounds and list lengths):
//   quantise_bounds  one lane per pixel: q, the face and E bits into one packed word, the output value; the six bounds by a wave-level
//                    maximum and one atomicMax per bound and wave that holds an eye pixel (a minimum m is kept as BOUND_TOP - m: zero is empty)
//   erode            one lane per pixel of the band, rows [h/4 - 4, h/2 + 4): P, the 81 offsets of the disc against E, the F and M bits
//   columns          one wave per (frame, column): the four column statistics by wave reductions, lo and hi, and the coordinates
//                    of B and of F appended to the frame's two lists, one atomicAdd per wave and list.  The lists' order is arbitrary;
//                    nothing downstream depends on it.
//   fill             64 blink pixels per block of four waves, ONE LANE per pixel in each wave; the face list passes through LDS in tiles of
//                    512 coordinates, each wave scanning a quarter of every tile, 16 bytes per read, every lane at the same address (a
//                    broadcast): the minimum over the 64-bit key needs no exchange between lanes, only one of four partial minima
//                    per pixel through LDS at the end.  Wave 0 writes the three output values.  Block 0 of each frame writes the status word.
// B and F are disjoint, so fill reads the colours of F and writes only pixels of B: in place is safe, and there is no separate finishing pass.
#include "r3d_common.h"

namespace r3d {
namespace blink {

constexpr int MIN_SIZE = 16, MAX_SIZE = 4096, MAX_FRAMES = 65535;          // h, w >= 16: min_h - 4 and lmin - 4 cannot go negative; F: gridDim.y
constexpr int ROOM = 4, R2 = 25, RAD = 5;
constexpr unsigned BOUND_TOP = 0x10000u;          // a minimum m is stored as BOUND_TOP - m, a maximum as m + 1: the memset's zero is "none"
constexpr unsigned FACE_BIT = 1u << 24, EYE_BIT = 1u << 25;
constexpr unsigned F_BIT = 1, M_BIT = 2;
constexpr size_t HEAD_BYTES = 256;                 // per frame: min_h, max_h, lmin, lmax, rmin, rmax, nF, nB
enum { H_MINH, H_MAXH, H_LMIN, H_LMAX, H_RMIN, H_RMAX, H_NF, H_NB };
constexpr int TILE = 512, FILL_PIXELS = 64, FILL_WAVES = 4, SLICE = TILE / FILL_WAVES, FILL_MAX_BLOCKS = 2048;

struct Args {
    const float* secc;                    // [T, 3, H, W]
    float* out;                           // [T, 3, H, W], may be secc
    const int* frame_idx;                 // [F]
    const double* percent;                // [F]
    int* status;                          // [F]
    int T, H, W, F;
    int band0, band;                      // the band's first row and its number of rows
    unsigned cap;                         // band x W: the capacity of each list
    unsigned* head;                       // [F, 64]
    unsigned* pix;                        // [F, H W]: q0 | q1 << 8 | q2 << 16 | FACE_BIT | EYE_BIT
    unsigned char* mask;                  // [F, band W]: F_BIT or M_BIT, 0 outside P
    unsigned* flist;                      // [F, cap]: row << 16 | col of F's pixels
    unsigned* blist;                      // [F, cap]: of B's
};

struct Box { int r0, r1, l0, l1, q0, q1; };          // P: rows [r0, r1), cols [l0, l1) u [q0, q1)

// the frame's index and percentage when both are acceptable
__device__ __forceinline__ bool frame_ok(const Args& a, int f, int& idx, double& p)
{
    idx = a.frame_idx[f];
    p = a.percent[f];
    return (unsigned)idx < (unsigned)a.T && p >= 0.0 && p <= 1.0;
}

// P from the frame's head; false when a prior region holds no eye pixel (status 1)
__device__ __forceinline__ bool load_box(const Args& a, const unsigned* head, Box& b)
{
    const unsigned e0 = head[H_MINH], e1 = head[H_MAXH], e2 = head[H_LMIN], e3 = head[H_LMAX], e4 = head[H_RMIN], e5 = head[H_RMAX];
    if (e2 == 0 || e3 == 0 || e4 == 0 || e5 == 0 || e0 == 0 || e1 == 0) return false;
    b.r0 = max((int)(BOUND_TOP - e0) - ROOM, 0); b.r1 = min((int)(e1 - 1) + ROOM, a.H);
    b.l0 = max((int)(BOUND_TOP - e2) - ROOM, 0); b.l1 = min((int)(e3 - 1) + ROOM, a.W);
    b.q0 = max((int)(BOUND_TOP - e4) - ROOM, 0); b.q1 = min((int)(e5 - 1) + ROOM, a.W);
    return true;
}

__device__ __forceinline__ bool in_cols(const Box& b, int c) { return (c >= b.l0 && c < b.l1) || (c >= b.q0 && c < b.q1); }

__device__ __forceinline__ unsigned wave_max(unsigned v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, s, 64));
    return v;
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__device__ __forceinline__ unsigned quantise(float v)
{
#pragma clang fp contract(off)
    const float t = ((v + 1.0f) * 0.5f) * 255.0f;                                      // (img + 1) / 2 * 255: the halving is exact
    return (unsigned)(int)fminf(fmaxf(t, 0.0f), 255.0f);                               // fmaxf(NaN, 0) = 0
}

__device__ __forceinline__ float dequantise(unsigned q)
{
#pragma clang fp contract(off)
    return (float)q / 127.5f - 1.0f;                                                   // hipcc's fp32 division is correctly rounded
}

// lo and hi of one column: two products and one sum each, every one rounded on its own as NumPy rounds them.  The _rn intrinsics are plain
// operators to this compiler, which would fuse them: contraction is switched off for the function instead.
__device__ __forceinline__ void column_limits(double p, int sum, int cnt, int mn, int mx, double& lo, double& hi)
{
#pragma clang fp contract(off)
    const double mean = (double)sum / (double)cnt, rest = 1.0 - p, pm = p * mean;
    const double a = rest * (double)mn, b = rest * (double)mx;
    lo = pm + a;
    hi = pm + b;
}

__global__ void __launch_bounds__(256) quantise_bounds(Args a)
{
    const int f = blockIdx.y;
    int idx; double p;
    if (!frame_ok(a, f, idx, p)) return;
    const size_t hw = (size_t)a.H * a.W, g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = g < hw;
    const int r = live ? (int)(g / a.W) : 0, c = live ? (int)(g - (size_t)r * a.W) : 0;
    bool eye = false, left = false;
    if (live) {
        const float* in = a.secc + (size_t)idx * 3 * hw + g;
        const unsigned q0 = quantise(in[0]), q1 = quantise(in[hw]), q2 = quantise(in[2 * hw]);          // read before the writes: out may be secc
        float* o = a.out + (size_t)idx * 3 * hw + g;
        o[0] = dequantise(q0); o[hw] = dequantise(q1); o[2 * hw] = dequantise(q2);
        const bool face = q0 != 0 && q1 != 0 && q2 != 0;
        const int w4 = a.W / 4;
        const bool rows = r >= a.H / 4 && r < a.H / 2;
        left = rows && c >= w4 && c < a.W / 2;
        const bool right = rows && c >= a.W / 2 && c < w4 * 3;
        eye = !face && (left || right);
        a.pix[(size_t)f * hw + g] = q0 | (q1 << 8) | (q2 << 16) | (face ? FACE_BIT : 0u) | (eye ? EYE_BIT : 0u);
    }
    if (p == 0.0 || __ballot(eye) == 0ull) return;          // wave-uniform
    unsigned* head = a.head + (size_t)f * (HEAD_BYTES / 4);
    const unsigned v0 = wave_max(eye ? BOUND_TOP - (unsigned)r : 0u), v1 = wave_max(eye ? (unsigned)r + 1u : 0u);
    const unsigned v2 = wave_max(eye && left ? BOUND_TOP - (unsigned)c : 0u), v3 = wave_max(eye && left ? (unsigned)c + 1u : 0u);
    const unsigned v4 = wave_max(eye && !left ? BOUND_TOP - (unsigned)c : 0u), v5 = wave_max(eye && !left ? (unsigned)c + 1u : 0u);
    if ((threadIdx.x & 63) == 0) {
        atomicMax(head + H_MINH, v0); atomicMax(head + H_MAXH, v1);
        if (v2) { atomicMax(head + H_LMIN, v2); atomicMax(head + H_LMAX, v3); }
        if (v4) { atomicMax(head + H_RMIN, v4); atomicMax(head + H_RMAX, v5); }
    }
}

__global__ void __launch_bounds__(256) erode(Args a)
{
    const int f = blockIdx.y;
    int idx; double p;
    if (!frame_ok(a, f, idx, p) || p == 0.0) return;
    Box b;
    if (!load_box(a, a.head + (size_t)f * (HEAD_BYTES / 4), b)) return;
    const unsigned g = blockIdx.x * 256 + threadIdx.x;
    if (g >= a.cap) return;
    const int r = a.band0 + (int)(g / (unsigned)a.W), c = (int)(g % (unsigned)a.W);
    const unsigned* pix = a.pix + (size_t)f * a.H * a.W;
    unsigned char m = 0;
    if (r >= b.r0 && r < b.r1 && in_cols(b, c)) {
        bool keep = (pix[(size_t)r * a.W + c] & FACE_BIT) != 0;
        if (keep) {
            const int y0 = max(r - RAD, 0), y1 = min(r + RAD, a.H - 1), x0 = max(c - RAD, 0), x1 = min(c + RAD, a.W - 1);
            for (int y = y0; y <= y1 && keep; ++y)
                for (int x = x0; x <= x1; ++x)
                    if ((y - r) * (y - r) + (x - c) * (x - c) <= R2 && (pix[(size_t)y * a.W + x] & EYE_BIT)) keep = false;
        }
        m = keep ? F_BIT : M_BIT;
    }
    a.mask[(size_t)f * a.cap + g] = m;
}

// this lane's slot among the lanes of the wave for which `take` holds, behind one atomicAdd of their number (every lane of the wave calls it)
__device__ __forceinline__ unsigned append_slot(unsigned* counter, bool take)
{
    const unsigned long long votes = __ballot(take);
    const unsigned lane = threadIdx.x & 63;
    unsigned base = 0;
    if (lane == 0 && votes) base = atomicAdd(counter, (unsigned)__popcll(votes));
    base = (unsigned)__shfl((int)base, 0, 64);
    return base + (unsigned)__popcll(votes & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(256) columns(Args a)
{
    const int f = blockIdx.y;
    int idx; double p;
    if (!frame_ok(a, f, idx, p) || p == 0.0) return;
    unsigned* head = a.head + (size_t)f * (HEAD_BYTES / 4);
    Box b;
    if (!load_box(a, head, b)) return;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= a.W || !in_cols(b, c)) return;                                   // wave-uniform
    const int r0 = max(b.r0, a.band0), r1 = min(b.r1, a.band0 + a.band);      // P lies inside the band; never index outside it
    const unsigned char* mask = a.mask + (size_t)f * a.cap;
    int cnt = 0, sum = 0;
    unsigned lo_enc = 0, hi_enc = 0;
    for (int r = r0 + lane; r < r1; r += 64)
        if (mask[(size_t)(r - a.band0) * a.W + c] & M_BIT) {
            ++cnt; sum += r;
            lo_enc = max(lo_enc, BOUND_TOP - (unsigned)r); hi_enc = max(hi_enc, (unsigned)r + 1u);
        }
    cnt = wave_sum(cnt); sum = wave_sum(sum);
    lo_enc = wave_max(lo_enc); hi_enc = wave_max(hi_enc);
    double lo = -1.0, hi = 1e9;                                               // cnt == 0: the column contributes nothing
    if (cnt > 0) column_limits(p, sum, cnt, (int)(BOUND_TOP - lo_enc), (int)(hi_enc - 1u), lo, hi);
    for (int base = r0; base < r1; base += 64) {                              // whole waves: append_slot votes
        const int r = base + lane;
        unsigned char m = 0;
        if (r < r1) m = mask[(size_t)(r - a.band0) * a.W + c];
        const bool blinks = (m & M_BIT) && ((double)r <= lo || (double)r >= hi);
        const unsigned rc = ((unsigned)r << 16) | (unsigned)c;
        const unsigned sb = append_slot(head + H_NB, blinks);
        if (blinks && sb < a.cap) a.blist[(size_t)f * a.cap + sb] = rc;
        const bool isf = (m & F_BIT) != 0;
        const unsigned sf = append_slot(head + H_NF, isf);
        if (isf && sf < a.cap) a.flist[(size_t)f * a.cap + sf] = rc;
    }
}

// the key (d^2, row, col) of the face pixel rc = row << 16 | col seen from (r, c), kept when smaller
__device__ __forceinline__ void nearer(unsigned rc, int r, int c, unsigned long long& best)
{
    const int dy = (int)(rc >> 16) - r, dx = (int)(rc & 0xffffu) - c;
    const unsigned long long key = ((unsigned long long)(unsigned)(dy * dy + dx * dx) << 32) | rc;
    best = key < best ? key : best;
}

__global__ void __launch_bounds__(FILL_PIXELS * FILL_WAVES) fill(Args a)
{
    __shared__ __attribute__((aligned(16))) unsigned tile[TILE];
    __shared__ unsigned long long part[FILL_WAVES][FILL_PIXELS];
    const int f = blockIdx.y;
    int idx; double p;
    const bool ok = frame_ok(a, f, idx, p);
    const unsigned* head = a.head + (size_t)f * (HEAD_BYTES / 4);
    Box b;
    const bool boxed = ok && p != 0.0 && load_box(a, head, b);
    const unsigned nf = boxed ? min(head[H_NF], a.cap) : 0u, nb = boxed ? min(head[H_NB], a.cap) : 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.status[f] = !ok ? 3 : p == 0.0 ? 0 : !boxed ? 1 : nf == 0 ? 2 : 0;
    if (nf == 0) return;
    const size_t hw = (size_t)a.H * a.W;
    const unsigned* pix = a.pix + (size_t)f * hw;
    const unsigned* flist = a.flist + (size_t)f * a.cap;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (unsigned first = blockIdx.x * FILL_PIXELS; first < nb; first += gridDim.x * FILL_PIXELS) {          // block-uniform
        const unsigned e = first + lane;
        const bool live = e < nb;
        const unsigned me = live ? a.blist[(size_t)f * a.cap + e] : 0u;
        const int r = (int)(me >> 16), c = (int)(me & 0xffffu);
        unsigned long long best = ~0ull;
        for (unsigned t0 = 0; t0 < nf; t0 += TILE) {
            const unsigned n = min((unsigned)TILE, nf - t0);
            __syncthreads();
            for (unsigned i = threadIdx.x; i < n; i += FILL_PIXELS * FILL_WAVES) tile[i] = flist[t0 + i];
            __syncthreads();
            const unsigned s1 = min(n, (wave + 1) * SLICE);          // this wave's quarter of the tile, 16-byte aligned
            unsigned i = wave * SLICE;
#pragma unroll 2
            for (; i + 4 <= s1; i += 4) {
                const uint4 v = *(const uint4*)(tile + i);
                nearer(v.x, r, c, best); nearer(v.y, r, c, best); nearer(v.z, r, c, best); nearer(v.w, r, c, best);
            }
            for (; i < s1; ++i) nearer(tile[i], r, c, best);
        }
        part[wave][lane] = best;
        __syncthreads();                                             // the next round writes `part` only behind the tile loop's barriers
        if (wave != 0 || !live) continue;
#pragma unroll
        for (int k = 1; k < FILL_WAVES; ++k) best = part[k][lane] < best ? part[k][lane] : best;
        const int sr = min((int)((unsigned)best >> 16), a.H - 1), sc = min((int)((unsigned)best & 0xffffu), a.W - 1);          // list entries lie in the image
        if (r >= a.H || c >= a.W) continue;
        const unsigned q = pix[(size_t)sr * a.W + sc];
        float* o = a.out + (size_t)idx * 3 * hw + (size_t)r * a.W + c;
        o[0] = dequantise(q & 255u); o[hw] = dequantise((q >> 8) & 255u); o[2 * hw] = dequantise((q >> 16) & 255u);
    }
}

// the sizes every entry point accepts; with a name the first miss is that entry point's message, without one
// (r3d_secc_blink_workspace_bytes, which knows no T and passes F) nothing is said
static bool sizes_ok(const char* what, int T, int F, int H, int W)
{
    auto no = [&](const char* fmt, auto... v) { if (what) set_error(fmt, what, v...); return false; };
    if (H < MIN_SIZE || H > MAX_SIZE || W < MIN_SIZE || W > MAX_SIZE) return no("%s: map size H = %d, W = %d is not in %d .. %d", H, W, MIN_SIZE, MAX_SIZE);
    if (T < 1 || F < 1 || F > T || F > MAX_FRAMES) return no("%s: F = %d selected frames of T = %d (1 <= F <= T, F <= %d)", F, T, MAX_FRAMES);
    return true;
}

inline size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }
inline int band_rows(int H) { return H / 2 - H / 4 + 2 * ROOM; }          // rows [H / 4 - 4, H / 2 + 4): inside the image for H >= 16

struct Layout { size_t head, pix, mask, flist, blist, total; };

inline Layout layout(int F, int H, int W)
{
    const size_t cap = (size_t)band_rows(H) * W;
    Layout l;
    l.head = 0;
    l.pix = (size_t)F * HEAD_BYTES;
    l.flist = l.pix + round256((size_t)F * H * W * 4);
    l.blist = l.flist + round256((size_t)F * cap * 4);
    l.mask = l.blist + round256((size_t)F * cap * 4);
    l.total = l.mask + round256((size_t)F * cap);
    return l;
}

enum { STAGE_CLEAR = 1, STAGE_QUANTISE = 2, STAGE_ERODE = 4, STAGE_COLUMNS = 8, STAGE_FILL = 16, STAGE_ALL = 31 };

static int run(const float* secc, int T, int H, int W, const int32_t* frame_idx, const double* percent, int F, float* out, int32_t* status,
               void* workspace, size_t workspace_bytes, int stages, hipStream_t st)
{
    if (!secc || !out || !frame_idx || !percent || !status)
        { set_error("secc_blink: NULL pointer (secc, frame_idx, percent, out and status are required)"); return R3D_ERR_INVALID_ARG; }
    if (!sizes_ok("secc_blink", T, F, H, W)) return R3D_ERR_INVALID_ARG;
    if (stages < 0 || stages > STAGE_ALL) { set_error("secc_blink: bad test-hook argument"); return R3D_ERR_INVALID_ARG; }
    const Layout l = layout(F, H, W);
    if (!workspace_ok("secc_blink", workspace, workspace_bytes, l.total, 8, "r3d_secc_blink_workspace_bytes")) return R3D_ERR_WORKSPACE;

    Args a;
    a.secc = secc; a.out = out; a.frame_idx = frame_idx; a.percent = percent; a.status = status;
    a.T = T; a.H = H; a.W = W; a.F = F;
    a.band0 = H / 4 - ROOM; a.band = band_rows(H); a.cap = (unsigned)((size_t)a.band * W);
    char* ws = (char*)workspace;
    a.head = (unsigned*)(ws + l.head); a.pix = (unsigned*)(ws + l.pix); a.mask = (unsigned char*)(ws + l.mask);
    a.flist = (unsigned*)(ws + l.flist); a.blist = (unsigned*)(ws + l.blist);

    ProfScope ps(R3D_PROF_MISC, st);
    if ((stages & STAGE_CLEAR) && hipMemsetAsync(a.head, 0, (size_t)F * HEAD_BYTES, st) != hipSuccess) return check_launch("secc_blink (clear)");
    const unsigned pixel_blocks = (unsigned)(((size_t)H * W + 255) / 256), band_blocks = (a.cap + 255) / 256;
    const unsigned fill_blocks = min((a.cap + FILL_PIXELS - 1) / FILL_PIXELS, (unsigned)FILL_MAX_BLOCKS);
    if (stages & STAGE_QUANTISE) hipLaunchKernelGGL(quantise_bounds, dim3(pixel_blocks, F), dim3(256), 0, st, a);
    if (stages & STAGE_ERODE) hipLaunchKernelGGL(erode, dim3(band_blocks, F), dim3(256), 0, st, a);
    if (stages & STAGE_COLUMNS) hipLaunchKernelGGL(columns, dim3((W + 3) / 4, F), dim3(256), 0, st, a);
    if (stages & STAGE_FILL) hipLaunchKernelGGL(fill, dim3(fill_blocks, F), dim3(FILL_PIXELS * FILL_WAVES), 0, st, a);
    return check_launch("secc_blink");
}

}  // namespace blink
}  // namespace r3d

using namespace r3d;

extern "C" size_t r3d_secc_blink_workspace_bytes(int F, int H, int W)
{
    return blink::sizes_ok(nullptr, F, F, H, W) ? blink::layout(F, H, W).total : 0;
}

extern "C" int r3d_secc_blink(const float* secc, int T, int H, int W, const int32_t* frame_idx, const double* percent, int F, float* out,
                              int32_t* status, void* workspace, size_t workspace_bytes, r3d_stream_t stream)
{
    return blink::run(secc, T, H, W, frame_idx, percent, F, out, status, workspace, workspace_bytes, blink::STAGE_ALL, (hipStream_t)stream);
}

// Test hook outside the C ABI of include/r3d_hip.h (OPTIONAL_SIGNATURES of real3dportrait_amd/_lib.py): the same call with only the stages of
// a bit mask run (1 clear, 2 quantise_bounds, 4 erode, 8 columns, 16 fill: scripts/prof_blink.py times them one by one).
extern "C" int r3d_debug_secc_blink(const float* secc, int T, int H, int W, const int32_t* frame_idx, const double* percent, int F, float* out,
                                    int32_t* status, void* workspace, size_t workspace_bytes, int stages, r3d_stream_t stream)
{
    return blink::run(secc, T, H, W, frame_idx, percent, F, out, status, workspace, workspace_bytes, stages, (hipStream_t)stream);
}
