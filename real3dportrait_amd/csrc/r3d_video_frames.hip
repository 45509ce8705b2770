// The clip's output video frames in out_mode 'concat_debug', inference only: what forward_secc2video does on the host after
// the frame loop (inference/real3d_infer.py:495-521) as one reduction over the clip's depth images and one pass that writes the strips.
//
// A strip [H, 5 W, 3] of bytes holds five H x W panels: ref | secc | raw | depth | image.  The bytes follow the reference's operators in
// their order and number formats (include/r3d_hip_video.h, rules (1) to (5)):
//   every panel ends in fp64: u -> clamp(u, -1, 1) -> ((u + 1) / 2) * 255 -> truncation; a NaN u is byte 0;
//   ref, raw, image   u = the fp32 value, widened;
//   secc              q = int32(trunc((s + 1) * 127.5)) in fp32, u = q / 127.5 - 1 in fp64 (the second quantisation is not the identity);
//   depth             u = ((d - min) / (max - min)) * 2 - 1 in fp32 with IEEE division, min and max of the whole clip from the state
//                     (the reference's are those of the up-sampled images, which hold the same values: a depth image that is larger
//                     than the frame is refused);
//   secc, raw, depth  are gathered with F.interpolate's legacy nearest rule: min(floor(dst * (float(in) / float(out))), in - 1) in fp32.
// Contraction into fused multiply-adds is off for the whole file: every product above is rounded before the sum that follows it.
//
// Composer: memory-bound, planar fp32 in, interleaved bytes out.  A lane owns PX consecutive pixels of one panel row: PX = 16 is four
// 16-byte loads per channel (one where the source is a quarter as wide, the product's raw and depth images) and three 16-byte stores;
// PX = 4, for W % 16 != 0 or a pointer that is not 16-byte aligned, is scalar loads and three dword stores.  No byte stores, no atomics,
// no LDS.  Consecutive lanes write consecutive 3 PX bytes of the strip row.
//
// Depth range: a grid-stride reduction to per-block (min, max, NaN seen) on the ordered-integer image of the values, which makes min and
// max exact and independent of order.  One lane per block folds its block's result into the state's partial words with integer atomics,
// then takes a ticket; the block that draws the last ticket folds the partial words into the state's result (or replaces it: reset) and
// leaves the partial words and the ticket zero for the next call.  Only atomics touch the words that blocks share within a launch.
#include <limits.h>

#include "r3d_common.h"

#pragma clang fp contract(off)

namespace r3d {
namespace video {

constexpr int THREADS = 256;
constexpr int RANGE_MAX_BLOCKS = 1024;
constexpr int RANGE_PER_THREAD = 16;           // floats a lane reads before the grid grows
constexpr int MAX_SIDE = 1 << 24;              // the nearest rule multiplies an index in fp32
enum { ST_MIN, ST_MAX, ST_NAN, ST_VALID, ST_TICKET, ST_PLO, ST_PHI, ST_PNAN };          // the words of the state
static_assert(ST_PNAN + 1 == R3D_VIDEO_STATE_WORDS, "the header's state size");

// fp32, not NaN -> an unsigned key of the same order (-0.0 below +0.0); neither 0 nor 0xffffffff, which stand for "no value"
__device__ __forceinline__ unsigned ukey(float v) { return (unsigned)f2ord(v) ^ 0x80000000u; }
__device__ __forceinline__ float ukey_value(unsigned u) { return ord2f((int)(u ^ 0x80000000u)); }

struct Range {
    unsigned lo = 0xffffffffu, hi = 0u, nan = 0u;          // smallest key, largest key, NaN seen
    __device__ __forceinline__ void take(float v)
    {
        if (v == v) { const unsigned k = ukey(v); lo = min(lo, k); hi = max(hi, k); }
        else nan = 1u;
    }
    __device__ __forceinline__ void merge(unsigned l, unsigned h, unsigned n) { lo = min(lo, l); hi = max(hi, h); nan |= n; }
};

__global__ void __launch_bounds__(THREADS) depth_range_kernel(const float* __restrict__ d, unsigned count, int vec, int reset, unsigned* state)
{
    __shared__ unsigned part[THREADS / 64][3];
    const unsigned tid = blockIdx.x * THREADS + threadIdx.x, stride = gridDim.x * THREADS;
    Range r;
    if (vec) {                                    // d is 16-byte aligned
        const unsigned n4 = count >> 2;
        const f32x4* d4 = reinterpret_cast<const f32x4*>(d);
        for (unsigned i = tid; i < n4; i += stride) {
            const f32x4 v = d4[i];
            r.take(v.x); r.take(v.y); r.take(v.z); r.take(v.w);
        }
        if (tid < (count & 3u)) r.take(d[(n4 << 2) + tid]);
    } else {
        for (unsigned i = tid; i < count; i += stride) r.take(d[i]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) r.merge(__shfl_xor(r.lo, m, 64), __shfl_xor(r.hi, m, 64), __shfl_xor(r.nan, m, 64));
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = r.lo; part[threadIdx.x >> 6][1] = r.hi; part[threadIdx.x >> 6][2] = r.nan; }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) r.merge(part[w][0], part[w][1], part[w][2]);
    // the partial words are zero between calls: the smallest key is kept as the largest complement
    if (r.hi != 0u) { atomicMax(state + ST_PLO, ~r.lo); atomicMax(state + ST_PHI, r.hi); }
    if (r.nan) atomicOr(state + ST_PNAN, 1u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");          // the atomics above are performed before the ticket is taken
    const unsigned ticket = __hip_atomic_fetch_add(state + ST_TICKET, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != gridDim.x - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    Range all;                                    // every block's atomics have been performed: read and re-arm in one step
    all.lo = ~atomicExch(state + ST_PLO, 0u);
    all.hi = atomicExch(state + ST_PHI, 0u);
    all.nan = atomicExch(state + ST_PNAN, 0u);
    atomicExch(state + ST_TICKET, 0u);
    if (!reset && state[ST_VALID]) {              // written by an earlier launch
        if (state[ST_NAN]) all.nan = 1u;
        else all.merge(ukey(__uint_as_float(state[ST_MIN])), ukey(__uint_as_float(state[ST_MAX])), 0u);
    }
    const unsigned qnan = 0x7fc00000u;            // torch.min / max of a tensor with a NaN
    state[ST_MIN] = all.nan ? qnan : __float_as_uint(ukey_value(all.lo));
    state[ST_MAX] = all.nan ? qnan : __float_as_uint(ukey_value(all.hi));
    state[ST_NAN] = all.nan;
    state[ST_VALID] = 1u;
}

struct ComposeArgs {
    const float *ref, *secc, *raw, *depth, *image;
    const int* state;
    uint8_t* out;
    int hs, ws, hr, wr, hd, wd, n, H, W, panels;
    float secc_sy, secc_sx, raw_sy, raw_sx, depth_sy, depth_sx;          // float(in) / float(out), rule (5)
};

// rule (5); in == out is the identity (ATen returns the index itself there)
__device__ __forceinline__ int nearest(int dst, float scale, int in, int out)
{
    return in == out ? dst : min((int)((float)dst * scale), in - 1);
}

// PX pixels from x0 on of a panel row gathered from a source row of in_w values
template <int PX>
__device__ __forceinline__ void gather_row(const float* __restrict__ row, int in_w, int W, float scale, int x0, float (&v)[PX])
{
    if (PX == 16 && in_w == W) {
        const f32x4* r4 = reinterpret_cast<const f32x4*>(row + x0);
#pragma unroll
        for (int k = 0; k < PX / 4; ++k) { const f32x4 f = r4[k]; v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w; }
    } else if (PX == 16 && 4 * in_w == W) {       // scale 0.25 exactly: pixel x reads x >> 2
        const f32x4 f = *reinterpret_cast<const f32x4*>(row + (x0 >> 2));
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = f.x; v[4 + k] = f.y; v[8 + k] = f.z; v[12 + k] = f.w; }
    } else {
#pragma unroll
        for (int j = 0; j < PX; ++j) v[j] = row[nearest(x0 + j, scale, in_w, W)];
    }
}

// rules (1) and (4).  ((c + 1) / 2) * 255 is written (c + 1) * 127.5: the halving is exact, so both round the same real number once
__device__ __forceinline__ unsigned quantise(double u)
{
    const double c = fmin(fmax(u, -1.0), 1.0);
    const double w = (c + 1.0) * 127.5;
    return u != u ? 0u : (unsigned)(int)w;
}

// the same for a value that is fp32: the clamp commutes with the exact widening, and -1 and 1 are fp32 numbers
__device__ __forceinline__ unsigned quantise(float x)
{
    const float c = fminf(fmaxf(x, -1.0f), 1.0f);
    const double w = ((double)c + 1.0) * 127.5;
    return x != x ? 0u : (unsigned)(int)w;
}

// rule (2), the first quantisation and the way back
__device__ __forceinline__ double secc_value(float s)
{
    const float p = (s + 1.0f) * 127.5f;
    const int q = fabsf(p) < 2147483648.0f ? (int)p : INT_MIN;
    return (double)q / 127.5 - 1.0;
}

template <int PX>
__global__ void __launch_bounds__(THREADS) compose_kernel(const ComposeArgs a)
{
    const unsigned G = (unsigned)a.W / PX, per_row = 5u * G, total = (unsigned)a.n * (unsigned)a.H * per_row;          // < 2^31 / (3 PX)
    const unsigned idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= total) return;
    const unsigned row = idx / per_row, in_row = idx - row * per_row, p = in_row / G, g = in_row - p * G;
    if (!((a.panels >> p) & 1)) return;
    const int t = (int)(row / (unsigned)a.H), y = (int)(row - (unsigned)t * (unsigned)a.H), x0 = (int)g * PX;
    const int H = a.H, W = a.W;
    unsigned words[3 * PX / 4];
#pragma unroll
    for (int k = 0; k < 3 * PX / 4; ++k) words[k] = 0u;
    float v[PX];
    if (p == 3) {                                 // depth: one channel on all three
        const float mn = __int_as_float(a.state[ST_MIN]), mx = __int_as_float(a.state[ST_MAX]), range = mx - mn;
        const int sy = nearest(y, a.depth_sy, a.hd, H);
        gather_row<PX>(a.depth + ((size_t)t * a.hd + sy) * a.wd, a.wd, W, a.depth_sx, x0, v);
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const float f = ((v[j] - mn) / range) * 2.0f - 1.0f;
            const unsigned b = quantise(f);
#pragma unroll
            for (int c = 0; c < 3; ++c) words[(3 * j + c) >> 2] |= b << (8 * ((3 * j + c) & 3));
        }
    } else {
        const float* src; int in_h, in_w, frame; float sy_scale, sx_scale;
        if (p == 0) { src = a.ref; in_h = H; in_w = W; frame = 0; sy_scale = 1.0f; sx_scale = 1.0f; }
        else if (p == 1) { src = a.secc; in_h = a.hs; in_w = a.ws; frame = t; sy_scale = a.secc_sy; sx_scale = a.secc_sx; }
        else if (p == 2) { src = a.raw; in_h = a.hr; in_w = a.wr; frame = t; sy_scale = a.raw_sy; sx_scale = a.raw_sx; }
        else { src = a.image; in_h = H; in_w = W; frame = t; sy_scale = 1.0f; sx_scale = 1.0f; }
        const int sy = nearest(y, sy_scale, in_h, H);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gather_row<PX>(src + (((size_t)frame * 3 + c) * in_h + sy) * in_w, in_w, W, sx_scale, x0, v);
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const unsigned b = p == 1 ? quantise(secc_value(v[j])) : quantise(v[j]);
                words[(3 * j + c) >> 2] |= b << (8 * ((3 * j + c) & 3));
            }
        }
    }
    uint8_t* o = a.out + ((size_t)row * 5 + p) * 3 * (size_t)W + (size_t)x0 * 3;
    if (PX == 16) {
        uint4* o4 = reinterpret_cast<uint4*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k) o4[k] = make_uint4(words[4 * k], words[4 * k + 1], words[4 * k + 2], words[4 * k + 3]);
    } else {
        unsigned* o1 = reinterpret_cast<unsigned*>(o);
#pragma unroll
        for (int k = 0; k < 3 * PX / 4; ++k) o1[k] = words[k];
    }
}

}  // namespace video
}  // namespace r3d

using namespace r3d;

extern "C" int r3d_video_depth_range(const float* depth, size_t count, int reset, int32_t* state, r3d_stream_t stream)
{
    const char* what = "video_depth_range";
    if (!depth || !state) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (count < 1) { set_error("%s: count = 0 must be positive", what); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31(what, "4 count", (double)count * 4.0, "bytes")) return R3D_ERR_INVALID_ARG;
    if (!aligned(state, 4)) { set_error("%s: the state is not 4-byte aligned", what); return R3D_ERR_INVALID_ARG; }
    const Span spans[] = {writes(state, R3D_VIDEO_STATE_WORDS), reads(depth, count)};
    if (clash(spans)) { set_error("%s: the state overlaps the input", what); return R3D_ERR_INVALID_ARG; }
    ProfScope ps(R3D_PROF_LAYOUT, (hipStream_t)stream);
    const size_t per_block = (size_t)video::THREADS * video::RANGE_PER_THREAD;
    size_t blocks = (count + per_block - 1) / per_block;
    if (blocks > (size_t)video::RANGE_MAX_BLOCKS) blocks = video::RANGE_MAX_BLOCKS;
    hipLaunchKernelGGL(video::depth_range_kernel, dim3((unsigned)blocks), dim3(video::THREADS), 0, (hipStream_t)stream, depth, (unsigned)count,
                       aligned16(depth) ? 1 : 0, reset, reinterpret_cast<unsigned*>(state));
    return check_launch(what);
}

extern "C" int r3d_video_compose_debug(const float* ref, const float* secc, int hs, int ws, const float* raw, int hr, int wr, const float* depth,
                                       int hd, int wd, const float* image, int n, int H, int W, int panels, const int32_t* state, uint8_t* out,
                                       r3d_stream_t stream)
{
    const char* what = "video_compose_debug";
    if (panels < 1 || panels > R3D_VIDEO_PANELS_ALL) { set_error("%s: panels = %d outside 1 .. %d", what, panels, R3D_VIDEO_PANELS_ALL); return R3D_ERR_INVALID_ARG; }
    const bool on[5] = {(panels & 1) != 0, (panels & 2) != 0, (panels & 4) != 0, (panels & 8) != 0, (panels & 16) != 0};
    if (!out || (on[0] && !ref) || (on[1] && !secc) || (on[2] && !raw) || (on[3] && (!depth || !state)) || (on[4] && !image)) {
        set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG;
    }
    if (n < 1 || H < 1 || W < 1 || (on[1] && (hs < 1 || ws < 1)) || (on[2] && (hr < 1 || wr < 1)) || (on[3] && (hd < 1 || wd < 1))) {
        set_error("%s: n = %d, H = %d, W = %d, secc %d x %d, raw %d x %d, depth %d x %d: every size must be positive", what, n, H, W, hs, ws, hr, wr, hd, wd);
        return R3D_ERR_INVALID_ARG;
    }
    if (W % 4 != 0) { set_error("%s: W = %d must be a multiple of 4 (a panel row of 3 W bytes is written in dwords)", what, W); return R3D_ERR_INVALID_ARG; }
    const int sides[8] = {H, W, on[1] ? hs : 1, on[1] ? ws : 1, on[2] ? hr : 1, on[2] ? wr : 1, on[3] ? hd : 1, on[3] ? wd : 1};
    for (int s : sides)
        if (s > video::MAX_SIDE) { set_error("%s: a side of %d pixels, the limit is 2^24 (the nearest rule's fp32 index)", what, s); return R3D_ERR_INVALID_ARG; }
    if (on[3]) {
        // the reference takes min and max of the RESIZED depth image (:504-506).  Nearest up-sampling repeats every source pixel, so the
        // source's range -- what the state holds -- is the image's; a source with pixels the resize drops has another one
        const int last_y = hd == H ? H - 1 : (int)((float)(H - 1) * ((float)hd / (float)H)), last_x = wd == W ? W - 1 : (int)((float)(W - 1) * ((float)wd / (float)W));
        if (hd > H || wd > W || last_y < hd - 1 || last_x < wd - 1) {
            set_error("%s: depth %d x %d is not up-sampled to %d x %d with every pixel used: the clip's depth range would not be the frames'", what, hd, wd, H, W);
            return R3D_ERR_INVALID_ARG;
        }
    }
    const double frame = (double)H * (double)W * 4.0;
    const double bytes[5] = {3.0 * frame, 12.0 * n * hs * (double)ws, 12.0 * n * hr * (double)wr, 4.0 * n * hd * (double)wd, 3.0 * n * frame};
    const double out_bytes = 15.0 * n * (double)H * (double)W;
    const void* srcs[5] = {ref, secc, raw, depth, image};
    const char* const panel[5] = {"panel 0, 12 H W", "panel 1, 12 n hs ws", "panel 2, 12 n hr wr", "panel 3, 4 n hd wd", "panel 4, 12 n H W"};
    if (!below_2_31(what, "15 n H W", out_bytes, "bytes of output")) return R3D_ERR_INVALID_ARG;
    for (int p = 0; p < 5; ++p)
        if (on[p] && !below_2_31(what, panel[p], bytes[p], "bytes")) return R3D_ERR_INVALID_ARG;
    if (!aligned(out, 4)) { set_error("%s: out is not 4-byte aligned", what); return R3D_ERR_INVALID_ARG; }
    if (on[3] && !aligned(state, 4)) { set_error("%s: the state is not 4-byte aligned", what); return R3D_ERR_INVALID_ARG; }
    Span spans[7] = {writes(out, (size_t)out_bytes), reads(state, on[3] ? R3D_VIDEO_STATE_WORDS : 0)};          // (a panel that is off: no bytes)
    for (int p = 0; p < 5; ++p) spans[2 + p] = Span{srcs[p], on[p] ? (size_t)bytes[p] : 0, false};
    if (clash(spans)) { set_error("%s: the output overlaps an input", what); return R3D_ERR_INVALID_ARG; }
    bool vec = W % 16 == 0 && aligned16(out);
    for (int p = 0; p < 5; ++p) vec = vec && (!on[p] || aligned16(srcs[p]));
    video::ComposeArgs a;
    a.ref = ref; a.secc = secc; a.raw = raw; a.depth = depth; a.image = image; a.state = reinterpret_cast<const int*>(state); a.out = out;
    a.hs = hs; a.ws = ws; a.hr = hr; a.wr = wr; a.hd = hd; a.wd = wd; a.n = n; a.H = H; a.W = W; a.panels = panels;
    a.secc_sy = (float)hs / (float)H; a.secc_sx = (float)ws / (float)W;
    a.raw_sy = (float)hr / (float)H; a.raw_sx = (float)wr / (float)W;
    a.depth_sy = (float)hd / (float)H; a.depth_sx = (float)wd / (float)W;
    ProfScope ps(R3D_PROF_LAYOUT, (hipStream_t)stream);
    const int px = vec ? 16 : 4;
    const size_t lanes = (size_t)n * H * 5 * (size_t)(W / px);
    const dim3 grid((unsigned)((lanes + video::THREADS - 1) / video::THREADS));
    if (vec) hipLaunchKernelGGL(video::compose_kernel<16>, grid, dim3(video::THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(video::compose_kernel<4>, grid, dim3(video::THREADS), 0, (hipStream_t)stream, a);
    return check_launch(what);
}
