// The frame loop's conditions from the source image and its segmap, inference only: what prepare_batch_from_inp builds on
// the host once per clip (inference/real3d_infer.py:244-260) -- the head image, inpaint_torso_job and extract_background(..., 'knn')
// (data_gen/utils/process_video/extract_segment_imgs.py:63-239) -- on uint8 and int32.  The rules, in the reference's order, are stated in
// include/r3d_hip_source.h; tests/source_conditions_ref.py restates them in NumPy.
//
// Nearest seed, exactly, in two passes.  column_pass: a lane per (frame, column, one of 8 row segments) walks down (into scratch), then
// up, the segments stitched through LDS, and leaves per pixel the row of
// the nearest seed of its own column (the one above on a tie, -1 without one).  row_pass: a block owns 256 pixels of a row, stages the
// row's W candidates in LDS as (seed row << 11 | c, dy^2) and every lane takes the minimum over c of the 64-bit key
// ((x - c)^2 + dy^2) << 32 | seed row << 11 | c: distance, then row, then column.  All lanes read the same LDS address (a broadcast).
// A column's candidates at its own minimum distance are its nearest seed above and below and the one above has the lower row, so this is
// the lexicographic minimum over all seeds.  H W W key evaluations per frame.
//
// Everything else is one lane per 4 consecutive pixels of the flattened image and dword stores (bytes only for the last H W % 4 pixels).
// No atomics but the status flags (integer OR), no floating point but the darkening product (fp64, one multiplication, truncated) and
// the final (x - 127.5f) / 127.5f.
#include <limits.h>

#include "r3d_common.h"

#pragma clang fp contract(off)

namespace r3d {
namespace source {

constexpr int THREADS = 256;
constexpr int COLS = 32, SEGS = THREADS / COLS;          // the column kernels: columns of a block, row segments of a column
constexpr int MAX_SIDE = R3D_SOURCE_MAX_SIDE;
constexpr int MAX_FRAMES = 65535;               // the row pass has a frame per grid z
constexpr unsigned NO_SEED = 1u << 30;          // dy^2 of a column without a seed: above every d2 (< 2^23), and the sum cannot overflow
constexpr int TORSO_L = 9, NECK_L = R3D_SOURCE_DARKEN, PUSH_DOWN = 4, DILATE = 3;
static_assert(MAX_SIDE == 1 << 11, "the key keeps a row and a column in 11 bits each");

static size_t pad16(size_t n) { return (n + 15) & ~(size_t)15; }

// the workspace of include/r3d_hip_source.h
struct Layout {
    size_t seed_rows, d2, index, sure, stage, cols, total;
    Layout(int B, int H, int W)
    {
        const size_t N = (size_t)H * W;
        seed_rows = 0;
        d2 = seed_rows + pad16(4 * B * N);
        index = d2 + pad16(4 * B * N);
        sure = index + pad16(4 * N);
        stage = sure + pad16(N);
        cols = stage + pad16(3 * N);
        total = cols + pad16(8 * (size_t)W);
    }
};

// the nearer of a column's seed rows above (or on) and below (or on) row r, the one above on a tie; -1: none
__device__ __forceinline__ int pick_row(int above, int next, int r) { return above < 0 || (next >= 0 && next - r < r - above) ? next : above; }

// A block owns COLS adjacent columns (lanes of a wave half: adjacent bytes of a mask row) and cuts them into SEGS row segments, a lane per
// (segment, column): the walks are latency-bound, so rows are walked in parallel and the segments stitched through LDS.
__global__ void __launch_bounds__(THREADS) column_pass(const uint8_t* __restrict__ mask, int invert, int B, int H, int W, int* __restrict__ above_row,
                                                       int* __restrict__ seed_row)
{
    __shared__ int firsts[SEGS][COLS], lasts[SEGS][COLS];
    const int col = threadIdx.x % COLS, g = threadIdx.x / COLS, idx = blockIdx.x * COLS + col;
    const bool active = idx < B * W;              // (every lane reaches the barrier)
    const int b = active ? idx / W : 0, c = active ? idx - b * W : 0;
    const int per = (H + SEGS - 1) / SEGS, r0 = active ? min(g * per, H) : 0, r1 = active ? min(r0 + per, H) : 0;
    const size_t base = (size_t)b * H * W + c;
    const uint8_t* m = mask + base;
    int *up = above_row + base, *s = seed_row + base;
    // down: the nearest seed above (or on) each row INSIDE the segment, into scratch; both walks are unrolled, their loads do not depend
    // on each other, only `last` / `next` is carried, and the two arrays are distinct
    int last = -1, first = -1;
#pragma unroll 8
    for (int r = r0; r < r1; ++r) {
        const bool seed = (m[(size_t)r * W] != 0) != (invert != 0);
        last = seed ? r : last;
        first = seed && first < 0 ? r : first;
        up[(size_t)r * W] = last;
    }
    firsts[g][col] = first;
    lasts[g][col] = last;
    __syncthreads();
    int last_in = -1, next = -1;                  // the nearest seed of the segments above, and of those below
    for (int k = 0; k < g; ++k) last_in = max(last_in, lasts[k][col]);
    for (int k = SEGS - 1; k > g; --k) next = firsts[k][col] >= 0 ? firsts[k][col] : next;
    int r = r1 - 1;
    for (; r >= r0 + 7; r -= 8) {                 // eight rows' loads first (written out: the compiler keeps each load behind the store before it)
        uint8_t mv[8];
        int av[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { mv[u] = m[(size_t)(r - u) * W]; av[u] = up[(size_t)(r - u) * W]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            next = (mv[u] != 0) != (invert != 0) ? r - u : next;
            s[(size_t)(r - u) * W] = pick_row(av[u] < 0 ? last_in : av[u], next, r - u);
        }
    }
    for (; r >= r0; --r) {
        next = (m[(size_t)r * W] != 0) != (invert != 0) ? r : next;
        const int above = up[(size_t)r * W];
        s[(size_t)r * W] = pick_row(above < 0 ? last_in : above, next, r);
    }
}

// best = min(best, the key of candidate k at horizontal offset dx).  |dx| < 2^11: ONE 24-bit multiply-add, written out (from dx * dx the
// compiler makes a 64-bit multiply-add and two moves, from __mul24 it adds a sign extension per evaluation)
__device__ __forceinline__ void take(unsigned long long& best, uint2 k, int dx)
{
    unsigned d2;
    asm("v_mad_i32_i24 %0, %1, %1, %2" : "=v"(d2) : "v"(dx), "v"(k.y));
    const unsigned long long key = ((unsigned long long)d2 << 32) | k.x;
    best = key < best ? key : best;
}

__global__ void __launch_bounds__(THREADS) row_pass(const int* __restrict__ seed_row, int H, int W, int* __restrict__ d2_out, int* __restrict__ index_out,
                                                    int* status_word)
{
    __shared__ uint2 cand[MAX_SIDE];
    const int r = blockIdx.y, b = blockIdx.z;
    const size_t row = ((size_t)b * H + r) * W;
    for (int c = threadIdx.x; c < W; c += THREADS) {
        const int sr = seed_row[row + c], dy = sr - r;
        cand[c] = sr < 0 ? make_uint2(0u, NO_SEED) : make_uint2(((unsigned)sr << 11) | (unsigned)c, (unsigned)(dy * dy));          // (low, high) word of the key at x = c
    }
    __syncthreads();
    const int x = blockIdx.x * THREADS + threadIdx.x;
    if (x >= W) return;
    unsigned long long best = ~0ull;
    int c = 0;
    for (; c + 8 <= W; c += 8) {                  // (unrolled by hand: the compiler does not unroll a loop around the asm)
#pragma unroll
        for (int u = 0; u < 8; ++u) take(best, cand[c + u], x - c - u);
    }
    for (; c < W; ++c) take(best, cand[c], x - c);
    const unsigned d2 = (unsigned)(best >> 32), lo = (unsigned)best;
    const bool none = d2 >= NO_SEED;
    if (d2_out) d2_out[row + x] = none ? INT_MAX : (int)d2;
    if (index_out) index_out[row + x] = none ? -1 : (int)(lo >> 11) * W + (int)(lo & 2047u);
    if (none && r == 0 && x == 0) atomicOr(status_word, 1);
}

// 4 pixels of 3 bytes / of 1 byte from p0 on, of an image of N pixels; the base is 4-byte aligned
__device__ __forceinline__ void store_rgb4(uint8_t* base, int p0, int N, const unsigned (&w)[3])
{
    if (p0 + 4 <= N) {
        unsigned* o = reinterpret_cast<unsigned*>(base + (size_t)p0 * 3);
        o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
    } else {
        for (int k = 0; k < 3 * (N - p0); ++k) base[(size_t)p0 * 3 + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}
__device__ __forceinline__ void store_mask4(uint8_t* base, int p0, int N, unsigned w)
{
    if (p0 + 4 <= N) *reinterpret_cast<unsigned*>(base + p0) = w;
    else for (int k = 0; k < N - p0; ++k) base[p0 + k] = (uint8_t)(w >> (8 * k));
}
__device__ __forceinline__ void put_rgb(unsigned (&w)[3], int j, int ch, unsigned byte) { w[(3 * j + ch) >> 2] |= byte << (8 * ((3 * j + ch) & 3)); }

// extract_background :118-133: the largest d2 over the frames, the first frame that reaches it, the sure mask and the sure pixels' colours
__global__ void __launch_bounds__(THREADS) background_combine(const uint8_t* __restrict__ img, const int* __restrict__ d2, int B, int N,
                                                              uint8_t* __restrict__ sure, uint8_t* __restrict__ stage)
{
    const int p0 = 4 * (blockIdx.x * THREADS + threadIdx.x);
    if (p0 >= N) return;
    unsigned w[3] = {0u, 0u, 0u}, m = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + j;
        if (p >= N) break;
        int best = -1, f = 0;
        for (int b = 0; b < B; ++b) {
            const int d = d2[(size_t)b * N + p];
            if (d > best) { best = d; f = b; }
        }
        if (best > 100) {
            m |= 1u << (8 * j);
            const uint8_t* px = img + ((size_t)f * N + p) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) put_rgb(w, j, ch, px[ch]);
        }
    }
    store_mask4(sure, p0, N, m);
    store_rgb4(stage, p0, N, w);
}

// :135-142: a pixel that is not sure copies the colour of its nearest sure pixel
__global__ void __launch_bounds__(THREADS) background_fill(const uint8_t* __restrict__ stage, const uint8_t* __restrict__ sure,
                                                           const int* __restrict__ index, int N, uint8_t* __restrict__ out)
{
    const int p0 = 4 * (blockIdx.x * THREADS + threadIdx.x);
    if (p0 >= N) return;
    unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + j;
        if (p >= N) break;
        const int src = sure[p] ? p : index[p];
        if (src < 0 || src >= N) continue;          // no sure pixel at all (status word 1): 0
        const uint8_t* px = stage + (size_t)src * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) put_rgb(w, j, ch, px[ch]);
    }
    store_rgb4(out, p0, N, w);
}

struct TorsoArgs {
    const uint8_t *img, *seg;
    int* cols;
    uint8_t *stage, *torso_img, *torso_mask, *with_bg_img, *with_bg_mask;
    int H, W, N;
    int weights[5];
    double darken[NECK_L];
};

__device__ __forceinline__ bool is_head(const uint8_t* seg, int N, int p) { return (seg[(size_t)N + p] | seg[(size_t)3 * N + p] | seg[(size_t)5 * N + p]) != 0; }

// inpaint_torso_job :157-170, :189-206 per column: record 0 the top torso pixel's row where the pixel above it is head, record 1 the pushed-down
// top row of the dilated neck where the pixel above its top is head; -1 otherwise
__global__ void __launch_bounds__(THREADS) torso_columns(const uint8_t* __restrict__ seg, int H, int W, int* __restrict__ cols)
{
    __shared__ int t_firsts[SEGS][COLS], d_firsts[SEGS][COLS], d_counts[SEGS][COLS];
    const int col = threadIdx.x % COLS, g = threadIdx.x / COLS, c = blockIdx.x * COLS + col;
    const bool active = c < W;                    // (every lane reaches the barrier)
    const int N = H * W, per = (H + SEGS - 1) / SEGS, r0 = active ? min(g * per, H) : 0, r1 = active ? min(r0 + per, H) : 0;
    const uint8_t *neck = seg + (size_t)2 * N + (active ? c : 0), *torso = seg + (size_t)4 * N + (active ? c : 0);
    // a row is in the dilated neck where one of the rows r - 3 .. r + 3 inside the image is neck: a 7-bit window that slides down
    unsigned window = 0u;
    for (int rr = r0 - DILATE; rr < r0 + DILATE && r0 < r1; ++rr) window = (window << 1) | (unsigned)(rr >= 0 && rr < H && neck[(size_t)rr * W] != 0);
    int t_first = -1, d_first = -1, d_count = 0;
#pragma unroll 8
    for (int r = r0; r < r1; ++r) {
        const int rr = min(r + DILATE, H - 1);    // (unconditional loads: the unrolled ones go out together)
        const uint8_t tv = torso[(size_t)r * W], nv = neck[(size_t)rr * W];
        window = ((window << 1) | (unsigned)(r + DILATE < H && nv != 0)) & 0x7fu;
        t_first = tv && t_first < 0 ? r : t_first;
        d_first = window && d_first < 0 ? r : d_first;
        d_count += window ? 1 : 0;
    }
    t_firsts[g][col] = t_first; d_firsts[g][col] = d_first; d_counts[g][col] = d_count;
    __syncthreads();
    if (g != 0 || !active) return;
    int t_top = -1, n_top = -1, count = 0;
    for (int k = SEGS - 1; k >= 0; --k) {
        t_top = t_firsts[k][col] >= 0 ? t_firsts[k][col] : t_top;
        n_top = d_firsts[k][col] >= 0 ? d_firsts[k][col] : n_top;
        count += d_counts[k][col];
    }
    const bool t_keep = t_top >= 1 && is_head(seg, N, (t_top - 1) * W + c);
    const bool n_keep = n_top >= 1 && is_head(seg, N, (n_top - 1) * W + c);
    cols[c] = t_keep ? t_top : -1;
    cols[W + c] = n_keep ? n_top + min(count - 1, PUSH_DOWN) : -1;
}

// is row r of a column inside the L rows painted upward from row `from` (-1: the column is not painted)?
__device__ __forceinline__ bool painted(int from, int r, int L) { return from >= 0 && r <= from && r > from - L; }

// :153-154, :171-182, :207-218: the image with its head at 0, the torso paint and the neck paint over it
__global__ void __launch_bounds__(THREADS) torso_paint(const TorsoArgs a)
{
    __shared__ double darken[NECK_L];
    if (threadIdx.x < NECK_L) darken[threadIdx.x] = a.darken[threadIdx.x];
    __syncthreads();
    const int p0 = 4 * (blockIdx.x * THREADS + threadIdx.x), N = a.N, W = a.W;
    if (p0 >= N) return;
    unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + j;
        if (p >= N) break;
        const int r = p / W, c = p - r * W, t = a.cols[c], n = a.cols[W + c];
        const int from = painted(n, r, NECK_L) ? n : painted(t, r, TORSO_L) ? t : -1;
        if (from >= 0) {
            const double s = darken[from - r];
            const uint8_t* px = a.img + ((size_t)from * W + c) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) put_rgb(w, j, ch, (unsigned)(int)((double)px[ch] * s));
        } else if (!is_head(a.seg, N, p)) {
            const uint8_t* px = a.img + (size_t)p * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) put_rgb(w, j, ch, px[ch]);
        }
    }
    store_rgb4(a.stage, p0, N, w);
}

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

// :219-239: the blur inside the neck paint mask, the two masks and the two images
__global__ void __launch_bounds__(THREADS) torso_blur_masks(const TorsoArgs a)
{
    const int p0 = 4 * (blockIdx.x * THREADS + threadIdx.x), N = a.N, W = a.W, H = a.H;
    if (p0 >= N) return;
    unsigned wt[3] = {0u, 0u, 0u}, wb[3] = {0u, 0u, 0u}, mt = 0u, mb = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + j;
        if (p >= N) break;
        const int r = p / W, c = p - r * W;
        const bool neck_paint = painted(a.cols[W + c], r, NECK_L), torso_paint = painted(a.cols[c], r, TORSO_L);
        unsigned neck = 0u;
        for (int rr = max(r - DILATE, 0); rr <= min(r + DILATE, H - 1); ++rr) neck |= a.seg[(size_t)2 * N + rr * W + c];
        const bool in_torso = neck != 0u || a.seg[(size_t)4 * N + p] != 0 || neck_paint || torso_paint;
        const bool in_bg = in_torso || a.seg[p] != 0;
        unsigned v[3];
        if (neck_paint) {
            int rows[5], cs[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) { rows[k] = reflect101(r + k - 2, H); cs[k] = reflect101(c + k - 2, W); }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                unsigned sum = 0u;
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    unsigned h = 0u;          // at most 255 * 256: the 16-bit horizontal sum
#pragma unroll
                    for (int i = 0; i < 5; ++i) h += (unsigned)a.weights[i] * a.stage[((size_t)rows[k] * W + cs[i]) * 3 + ch];
                    sum += (unsigned)a.weights[k] * h;
                }
                v[ch] = (sum + 32768u) >> 16;
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch] = a.stage[(size_t)p * 3 + ch];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            put_rgb(wb, j, ch, v[ch]);
            if (in_torso) put_rgb(wt, j, ch, v[ch]);
        }
        if (in_torso) mt |= 1u << (8 * j);
        if (in_bg) mb |= 1u << (8 * j);
    }
    store_rgb4(a.torso_img, p0, N, wt);
    store_rgb4(a.with_bg_img, p0, N, wb);
    store_mask4(a.torso_mask, p0, N, mt);
    store_mask4(a.with_bg_mask, p0, N, mb);
}

// does pixel p belong to one of the classes of the bit mask?
__device__ __forceinline__ bool selected(const uint8_t* seg, int classes, int N, int p)
{
    unsigned any = 0u;
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if ((classes >> k) & 1) any |= seg[(size_t)k * N + p];
    return any != 0u;
}

// _seg_out_img_with_segmap: the image with every pixel outside the selection at 0, and the selection
__global__ void __launch_bounds__(THREADS) select(const uint8_t* __restrict__ img, const uint8_t* __restrict__ seg, int classes, int N,
                                                  uint8_t* __restrict__ out, uint8_t* __restrict__ mask)
{
    const int p0 = 4 * (blockIdx.x * THREADS + threadIdx.x);
    if (p0 >= N) return;
    unsigned w[3] = {0u, 0u, 0u}, m = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + j;
        if (p >= N) break;
        if (!selected(seg, classes, N, p)) continue;
        m |= 1u << (8 * j);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) put_rgb(w, j, ch, img[(size_t)p * 3 + ch]);
    }
    store_rgb4(out, p0, N, w);
    if (mask) store_mask4(mask, p0, N, m);
}

__global__ void __launch_bounds__(THREADS) to_planes(const uint8_t* __restrict__ img, const uint8_t* __restrict__ seg, int classes, int N, int vec,
                                                     float* __restrict__ out)
{
    const int p0 = 4 * (blockIdx.x * THREADS + threadIdx.x);
    if (p0 >= N) return;
    float v[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = min(p0 + j, N - 1);
        const bool on = !seg || selected(seg, classes, N, p);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch][j] = ((float)(on ? img[(size_t)p * 3 + ch] : (uint8_t)0) - 127.5f) / 127.5f;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float* o = out + (size_t)ch * N + p0;
        if (vec) {                                // N % 4 == 0 and out is 16-byte aligned
            f32x4 q; q.x = v[ch][0]; q.y = v[ch][1]; q.z = v[ch][2]; q.w = v[ch][3];
            *reinterpret_cast<f32x4*>(o) = q;
        } else {
            for (int j = 0; j < 4 && p0 + j < N; ++j) o[j] = v[ch][j];
        }
    }
}

// ---- the host side: every check runs before any HIP call --------------------------------------------------------------------------------
// the sizes every entry point accepts (min_side: 3 where the blur reflects 2 pixels); with a name the first miss is that entry point's
// message, without one (r3d_source_workspace_bytes) nothing is said
static bool sizes_ok(const char* what, int B, int H, int W, int min_side)
{
    auto no = [&](const char* fmt, auto... v) { if (what) set_error(fmt, what, v...); return false; };
    if (B < 1 || H < 1 || W < 1) return no("%s: B = %d, H = %d, W = %d: every size must be positive", B, H, W);
    if (H < min_side || W < min_side) return no("%s: H = %d, W = %d: a side below %d (the blur reflects 2 pixels)", H, W, min_side);
    if (B > MAX_FRAMES) return no("%s: B = %d frames, above %d (a grid dimension)", B, MAX_FRAMES);
    if (H > MAX_SIDE || W > MAX_SIDE) return no("%s: H = %d, W = %d: a side above %d (the key holds 11 bits of a row and of a column)", H, W, MAX_SIDE);
    return below_2_31(what, "4 B H W", 4.0 * B * (double)H * (double)W, "bytes");
}

static bool workspace_ok(const char* what, const void* ws, size_t ws_bytes, const Layout& L)
{
    return r3d::workspace_ok(what, ws, ws_bytes, L.total, 16, "r3d_source_workspace_bytes", true);          // (alignment first, then the size)
}

static unsigned blocks_for(size_t lanes) { return (unsigned)((lanes + THREADS - 1) / THREADS); }

// `above` is scratch of the column pass, as large as seed_rows: the workspace's d2 part, which nothing else holds while the pass runs
static void launch_transform(const uint8_t* mask, int invert, int B, int H, int W, int* above, int* seed_rows, int* d2, int* index, int* status_word,
                             hipStream_t st)
{
    hipLaunchKernelGGL(column_pass, dim3((unsigned)(((size_t)B * W + COLS - 1) / COLS)), dim3(THREADS), 0, st, mask, invert, B, H, W, above, seed_rows);
    hipLaunchKernelGGL(row_pass, dim3(blocks_for(W), H, B), dim3(THREADS), 0, st, seed_rows, H, W, d2, index, status_word);
}

}  // namespace source
}  // namespace r3d

using namespace r3d;

extern "C" size_t r3d_source_workspace_bytes(int B, int H, int W)
{
    return source::sizes_ok(nullptr, B, H, W, 1) ? source::Layout(B, H, W).total : 0;
}

extern "C" int r3d_source_nearest(const uint8_t* mask, int B, int H, int W, int32_t* d2, int32_t* index, int32_t* status, void* workspace,
                                  size_t workspace_bytes, r3d_stream_t stream)
{
    const char* what = "source_nearest";
    if (!mask || !status || !workspace || (!d2 && !index)) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (!source::sizes_ok(what, B, H, W, 1)) return R3D_ERR_INVALID_ARG;
    if (!aligned(d2, 4) || !aligned(index, 4) || !aligned(status, 4)) { set_error("%s: d2, index or the status is not 4-byte aligned", what); return R3D_ERR_INVALID_ARG; }
    const source::Layout L(B, H, W);
    if (!source::workspace_ok(what, workspace, workspace_bytes, L)) return R3D_ERR_INVALID_ARG;
    const size_t n = (size_t)B * H * W;
    const Span spans[] = {reads(mask, n), writes(d2, n), writes(index, n), writes(status, R3D_SOURCE_STATUS_WORDS), {workspace, L.total, true}};
    if (clash(spans)) { set_error("%s: an output, the status or the workspace overlaps another array", what); return R3D_ERR_INVALID_ARG; }
    ProfScope ps(R3D_PROF_LAYOUT, (hipStream_t)stream);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    if (hipMemsetAsync(status, 0, 4 * R3D_SOURCE_STATUS_WORDS, st) != hipSuccess) return check_launch(what);
    source::launch_transform(mask, 0, B, H, W, reinterpret_cast<int*>(ws + L.d2), reinterpret_cast<int*>(ws + L.seed_rows), d2, index, status, st);
    return check_launch(what);
}

extern "C" int r3d_source_background(const uint8_t* img, const uint8_t* bg, int B, int H, int W, uint8_t* out, int32_t* status, void* workspace,
                                     size_t workspace_bytes, r3d_stream_t stream)
{
    const char* what = "source_background";
    if (!img || !bg || !out || !status || !workspace) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (!source::sizes_ok(what, B, H, W, 1)) return R3D_ERR_INVALID_ARG;
    if (!aligned(out, 4) || !aligned(status, 4)) { set_error("%s: out or the status is not 4-byte aligned", what); return R3D_ERR_INVALID_ARG; }
    const source::Layout L(B, H, W);
    if (!source::workspace_ok(what, workspace, workspace_bytes, L)) return R3D_ERR_INVALID_ARG;
    const size_t n = (size_t)H * W;
    const Span spans[] = {reads(img, 3 * n * B), reads(bg, n * B), writes(out, 3 * n), writes(status, R3D_SOURCE_STATUS_WORDS), {workspace, L.total, true}};
    if (clash(spans)) { set_error("%s: an output, the status or the workspace overlaps another array", what); return R3D_ERR_INVALID_ARG; }
    ProfScope ps(R3D_PROF_LAYOUT, (hipStream_t)stream);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    int *seed_rows = reinterpret_cast<int*>(ws + L.seed_rows), *d2 = reinterpret_cast<int*>(ws + L.d2), *index = reinterpret_cast<int*>(ws + L.index);
    const int N = H * W;
    const dim3 quads(source::blocks_for(((size_t)N + 3) / 4));
    if (hipMemsetAsync(status, 0, 4 * R3D_SOURCE_STATUS_WORDS, st) != hipSuccess) return check_launch(what);
    source::launch_transform(bg, 1, B, H, W, d2, seed_rows, d2, nullptr, status, st);          // (the row pass overwrites the scratch with d2)
    hipLaunchKernelGGL(source::background_combine, quads, dim3(source::THREADS), 0, st, img, d2, B, N, ws + L.sure, ws + L.stage);
    source::launch_transform(ws + L.sure, 0, 1, H, W, d2, seed_rows, nullptr, index, status + 1, st);          // (d2 has been consumed)
    hipLaunchKernelGGL(source::background_fill, quads, dim3(source::THREADS), 0, st, ws + L.stage, ws + L.sure, index, N, out);
    return check_launch(what);
}

extern "C" int r3d_source_torso(const uint8_t* img, const uint8_t* segmap, int H, int W, const double* darken, const int* blur_weights,
                                uint8_t* torso_img, uint8_t* torso_mask, uint8_t* with_bg_img, uint8_t* with_bg_mask, void* workspace,
                                size_t workspace_bytes, r3d_stream_t stream)
{
    const char* what = "source_torso";
    if (!img || !segmap || !darken || !blur_weights || !torso_img || !torso_mask || !with_bg_img || !with_bg_mask || !workspace) {
        set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG;
    }
    if (!source::sizes_ok(what, 1, H, W, 3)) return R3D_ERR_INVALID_ARG;
    int sum = 0;
    for (int k = 0; k < 5; ++k) {
        if (blur_weights[k] < 0 || blur_weights[k] > 256) { set_error("%s: blur weight %d = %d outside 0 .. 256", what, k, blur_weights[k]); return R3D_ERR_INVALID_ARG; }
        sum += blur_weights[k];
    }
    for (int k = 0; k < source::NECK_L; ++k)
        if (!(darken[k] >= 0.0 && darken[k] <= 1.0)) { set_error("%s: darken[%d] = %g outside 0 .. 1", what, k, darken[k]); return R3D_ERR_INVALID_ARG; }
    if (sum > 256) { set_error("%s: the blur weights sum to %d, above 256 (the horizontal sum has 16 bits)", what, sum); return R3D_ERR_INVALID_ARG; }
    if (!aligned(torso_img, 4) || !aligned(torso_mask, 4) || !aligned(with_bg_img, 4) || !aligned(with_bg_mask, 4)) {
        set_error("%s: an output is not 4-byte aligned", what); return R3D_ERR_INVALID_ARG;
    }
    const source::Layout L(1, H, W);
    if (!source::workspace_ok(what, workspace, workspace_bytes, L)) return R3D_ERR_INVALID_ARG;
    const size_t n = (size_t)H * W;
    const Span spans[] = {reads(img, 3 * n), reads(segmap, 6 * n), writes(torso_img, 3 * n), writes(torso_mask, n), writes(with_bg_img, 3 * n),
                          writes(with_bg_mask, n), {workspace, L.total, true}};
    if (clash(spans)) { set_error("%s: an output or the workspace overlaps another array", what); return R3D_ERR_INVALID_ARG; }
    ProfScope ps(R3D_PROF_LAYOUT, (hipStream_t)stream);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    source::TorsoArgs a;
    a.img = img; a.seg = segmap; a.cols = reinterpret_cast<int*>(ws + L.cols); a.stage = ws + L.stage;
    a.torso_img = torso_img; a.torso_mask = torso_mask; a.with_bg_img = with_bg_img; a.with_bg_mask = with_bg_mask;
    a.H = H; a.W = W; a.N = H * W;
    for (int k = 0; k < 5; ++k) a.weights[k] = blur_weights[k];
    for (int k = 0; k < source::NECK_L; ++k) a.darken[k] = darken[k];
    const dim3 quads(source::blocks_for(((size_t)a.N + 3) / 4));
    hipLaunchKernelGGL(source::torso_columns, dim3((unsigned)((W + source::COLS - 1) / source::COLS)), dim3(source::THREADS), 0, st, segmap, H, W, a.cols);
    hipLaunchKernelGGL(source::torso_paint, quads, dim3(source::THREADS), 0, st, a);
    hipLaunchKernelGGL(source::torso_blur_masks, quads, dim3(source::THREADS), 0, st, a);
    return check_launch(what);
}

extern "C" int r3d_source_select(const uint8_t* img, const uint8_t* segmap, int classes, int H, int W, uint8_t* out, uint8_t* mask, r3d_stream_t stream)
{
    const char* what = "source_select";
    if (!img || !segmap || !out) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (!source::sizes_ok(what, 1, H, W, 1)) return R3D_ERR_INVALID_ARG;
    if (classes < 1 || classes > 63) { set_error("%s: classes = %d outside 1 .. 63", what, classes); return R3D_ERR_INVALID_ARG; }
    if (!aligned(out, 4) || !aligned(mask, 4)) { set_error("%s: an output is not 4-byte aligned", what); return R3D_ERR_INVALID_ARG; }
    const size_t n = (size_t)H * W;
    const Span spans[] = {reads(img, 3 * n), reads(segmap, 6 * n), writes(out, 3 * n), writes(mask, n)};
    if (clash(spans)) { set_error("%s: an output overlaps another array", what); return R3D_ERR_INVALID_ARG; }
    ProfScope ps(R3D_PROF_LAYOUT, (hipStream_t)stream);
    const int N = H * W;
    hipLaunchKernelGGL(source::select, dim3(source::blocks_for(((size_t)N + 3) / 4)), dim3(source::THREADS), 0, (hipStream_t)stream, img, segmap, classes, N, out,
                       mask);
    return check_launch(what);
}

extern "C" int r3d_source_to_planes(const uint8_t* img, const uint8_t* segmap, int classes, int H, int W, float* out, r3d_stream_t stream)
{
    const char* what = "source_to_planes";
    if (!img || !out) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (!source::sizes_ok(what, 1, H, W, 1)) return R3D_ERR_INVALID_ARG;
    if (segmap && (classes < 1 || classes > 63)) { set_error("%s: classes = %d outside 1 .. 63", what, classes); return R3D_ERR_INVALID_ARG; }
    if (!aligned(out, 4)) { set_error("%s: out is not 4-byte aligned", what); return R3D_ERR_INVALID_ARG; }
    const size_t n = (size_t)H * W;
    const Span spans[] = {reads(img, 3 * n), reads(segmap, 6 * n), writes(out, 3 * n)};
    if (clash(spans)) { set_error("%s: the output overlaps an input", what); return R3D_ERR_INVALID_ARG; }
    ProfScope ps(R3D_PROF_LAYOUT, (hipStream_t)stream);
    const int N = H * W;
    hipLaunchKernelGGL(source::to_planes, dim3(source::blocks_for(((size_t)N + 3) / 4)), dim3(source::THREADS), 0, (hipStream_t)stream, img, segmap, classes, N,
                       (N % 4 == 0 && aligned16(out)) ? 1 : 0, out);
    return check_launch(what);
}
