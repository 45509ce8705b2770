// The implicit-GEMM stride-1 convolution of the torso network on v_mfma_f32_16x16x4_f32, shared by the 2-D kernels of
// r3d_torso.hip (torso_conv) and the 3-D ones of r3d_torso_motion.hip (conv3d): one body, conv_tile<VEC, D3, WM, WN, TM, TN>.
//
// A (WM TM 16) x (WN TN 16) tile of output positions x output channels per 256-thread block, K = (kz, ky, kx, ci) staged 32 at a time through
// two LDS buffers while the next two steps are in flight in registers.  Tap loads apply the prologue act(s[c] x + t[c]) (zero outside the image
// AFTER it: the reference pads the activated tensor) and nearest x2 up-sampling of H and W in the addressing; the epilogue adds the bias,
// applies LeakyReLU / sigmoid, adds a residual and writes channel-last and / or channel-first.  VEC: Cin % 4 == 0, channel-last input,
// 16-byte loads; otherwise one element per load.
//
// D3 = false is the 2-D convolution (D = 1, one depth tap): the depth fields of ConvArgs are not read and the code is the one r3d_torso_conv
// has always run.  D3 = true adds
//   * a depth tap: activations [B, D, Hs, Ws, Cin], weights [Cout, kd, ks, ks, Cin], zero padding padz in depth; the full-depth form is
//     kd = D, padz = 0, Do = 1 (a Conv2d over x.view(N, C D, H, W) whose weights were permuted on the host);
//   * AvgPool3d((1, 2, 2)) after the activation: the rows of a tile are enumerated quad-major (row 4 q + r is pixel (2 py + (r >> 1),
//     2 px + (r & 1)) of pooled position q), so the four accumulators a lane holds (rows 4 (lane >> 4) + r) are one window, averaged in the
//     epilogue; the un-pooled tensor is never written;
//   * an output channel stride and offset (a producer writes its slice of a concatenation);
//   * m-fast tile order for layers with fewer positions than output channels (every XCD streams its own share of the weights once).
//
// EXT = true (with D3; the appearance extractor's kernels, r3d_torso_appearance.hip) adds to that epilogue
//   * + residual [M, Cout] after the activation (may alias y: each element is read, then written, by one lane);
//   * the depth-split store of a 2-D layer (D = Do = 1): output channel n = d C + c, C = Cout / split, goes to [b, d, h, w, c] of a volume
//     [B, split, H, W, C] -- a Conv2d followed by x.view(N, C, D, H, W) whose weight rows the caller ordered depth-major.
// EXT = false compiles neither: the kernels of r3d_torso_conv3d are the code they were.
//
// DL = true (2-D, F32; the DeepLabV3 kernels of r3d_deeplab.hip) is nn.Conv2d with a stride, a dilation and an explicit padding:
//   * tap (ky, kx) of output (oy, ox) is input (oy cstride - cpad + ky cdil, ox cstride - cpad + kx cdil), tested against the stored Hs x Ws
//     (H x W is the OUTPUT grid; no up-sampling, no prologue, channel-last input only);
//   * the epilogue is BasicBlock's: sum + bias[b bias_bs + n], + residual [M, Cout] (may alias y), THEN ReLU (act 1), written to channels
//     [yco, yco + Cout) of rows of ycs floats.
// DL = false compiles none of it, and the four fields it reads travel in the depth words of ConvArgs, which a 2-D kernel does not read (ConvArgs::set_dl).
//
// RP = true (3-D with EXT, F32, VEC; the Plane2GridModule kernels of r3d_plane2grid.hip) is nn.Conv3d(padding_mode='replicate')
// behind a per-SAMPLE prologue, GroupNorm + ReLU as scale . x + shift:
//   * a tap's coordinates are clamped into the volume in depth, height and width, so every tap of a row that exists is inside;
//   * ps, pt are [B, Cin], and a tap is max(ps[b, c] x + pt[b, c], 0) with b the sample of ITS row (a tile's rows may belong to several
//     samples), a NaN stays a NaN; pslope is not read.  The pair travels with the row's slot in the stage.
// RP = false compiles none of it; ConvArgs is not touched.
//
// PREC selects the arithmetic of the products; loaders, tile order and epilogues are the same code for both.
//   F32     the fp32 operands as they are, 8 v_mfma_f32_16x16x4_f32 per 16 x 16 tile and k step.
//   BF16X3  store() splits every staged value into three bf16 pieces h + m + l == x (split_bf16x3) and compute() sums six of the nine
//           piece products on v_mfma_f32_16x16x32_bf16 into the same fp32 accumulators, smallest first:
//           l.h, h.l, m.m, m.h, h.m, h.h (activation piece . weight piece).  The dropped l.m, m.l, l.l are below 2^-25 of |x||w|.
//           bf16 has fp32's exponent: no range fold, no per-tensor state.
#pragma once
#include "r3d_common.h"
#include <math.h>
#include <type_traits>

namespace r3d {
namespace tconv {

constexpr int BK = 32, LDK = BK + 4;     // LDS rows of 36 floats: 16-byte aligned, and 16 rows at one k offset touch 64 distinct banks
constexpr int F32 = 0, BF16X3 = 1;       // PREC (R3D_TORSO_F32, R3D_TORSO_BF16X3)

// BF16X3's LDS row, in bf16 elements: [h: 32 k][m: 32 k][l: 32 k][8 of padding] = 208 bytes.  A piece's 32 k entries are four 16-byte slots,
// one per lane group of compute(); slot g of row r is stored at position g ^ bf3_swz(r).  ds_read_b128 serves 16 lanes at a time, rows
// {0-3, 12-15} of group g with rows {4-11} of group g + 1 (and the other way round): 13 r + (g ^ swz(r)) mod 16 takes 16 distinct values on
// either set, so every read touches each 16-byte slot of the 256-byte bank row once.  The 16 bytes of padding are for the element loader's
// 2-byte stores, where consecutive lanes write consecutive rows: 52 r mod 32 dwords takes 8 values (192-byte rows: 2).
constexpr int LDH = 3 * BK + 8;
__device__ __forceinline__ int bf3_swz(int row) { return ((row >> 2) ^ (row >> 3)) & 1; }
// the bf16 index of k entry k (0 .. 31) of piece p in row `row`
__device__ __forceinline__ int bf3_at(int row, int p, int k) { return row * LDH + p * BK + ((((k >> 3) ^ bf3_swz(row)) << 3) | (k & 7)); }

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- THE split of the BF16X3 tier: x == h + m + l exactly, three bf16 pieces (their 16 bits; a piece widened to fp32 is piece << 16).
//   h = bf16(clamp(x, -C, C)),  m = bf16(x - h),  l = bf16(x - h - m),  round-to-nearest-even, C = 0x7f7f0000 the largest finite bf16
// (without the clamp values above C would round to infinity; with it fp32 max splits exactly as well).  Both subtractions are exact in fp32:
// |x - h| <= ulp_bf16(x) / 2 has at most 16 significant bits, and after m at most 8 are left, so l is exact too -- down to |x| ~ 2^-110, where
// l (2^-16 |x|) falls below bf16's smallest normal and the matrix unit reads it as zero.  A non-finite x gives non-finite pieces (NaN for an
// infinity).  as_rounded(): the value is split as it was rounded to fp32, whatever produced it (a prologue multiply must not be contracted
// into the first subtraction at one use and not at another).  real3dportrait_amd/torso_precision.py:split_bf16x3 mirrors it bit for bit.
__device__ __forceinline__ void split_bf16x3(float x, uint16_t& h, uint16_t& m, uint16_t& l)
{
    x = as_rounded(x);
    const float big = __uint_as_float(0x7f7f0000u);
    const __bf16 hb = (__bf16)__builtin_amdgcn_fmed3f(x, -big, big);
    const float r1 = as_rounded(x - (float)hb);
    const __bf16 mb = (__bf16)r1;
    const float r2 = as_rounded(r1 - (float)mb);
    const __bf16 lb = (__bf16)r2;
    h = __builtin_bit_cast(uint16_t, hb); m = __builtin_bit_cast(uint16_t, mb); l = __builtin_bit_cast(uint16_t, lb);
}
// four consecutive k entries -> each piece's 8 bytes
__device__ __forceinline__ void split_bf16x3(const float4& v, uint2& h, uint2& m, uint2& l)
{
    uint16_t a[4], b[4], c[4];
    split_bf16x3(v.x, a[0], b[0], c[0]); split_bf16x3(v.y, a[1], b[1], c[1]);
    split_bf16x3(v.z, a[2], b[2], c[2]); split_bf16x3(v.w, a[3], b[3], c[3]);
    h = make_uint2(a[0] | (uint32_t)a[1] << 16, a[2] | (uint32_t)a[3] << 16);
    m = make_uint2(b[0] | (uint32_t)b[1] << 16, b[2] | (uint32_t)b[3] << 16);
    l = make_uint2(c[0] | (uint32_t)c[1] << 16, c[2] | (uint32_t)c[3] << 16);
}

struct ConvArgs {
    const float* x; int B, Hs, Ws, Cin;          // stored input [B, Hs, Ws, Cin] (in_nchw: [B, Cin, Hs, Ws]); D3: [B, D, Hs, Ws, Cin]
    int H, W;                                    // the conv's grid: Hs x Ws, or twice that (up: the input is x[h >> 1, w >> 1])
    int up, in_nchw, ks;
    int split;                                   // D3 and EXT only: > 1: the depth-split store, y [B, split, H, W, Cout / split] (D = Do = 1, no pool).
                                                 // It sits in what was padding in front of the next pointer: no other field moves, the struct keeps its size
    const float* ps; const float* pt; float pslope;      // prologue a = ps[c] x + pt[c]; a < 0 ? pslope a : a  (ps == nullptr: none)
    const float* w; int Cout;                    // [Cout, ks, ks, Cin]; D3: [Cout, kd, ks, ks, Cin]
    const float* bias;                           // [Cout] or nullptr
    int act; float slope;                        // 0 none, 1 v < 0 ? slope v : v, 2 sigmoid
    const float* res;                            // [M, Cout] or nullptr (may alias y: each element is read, then written, by one lane)
    float* y; float* y_nchw;                     // [B, H, W, Cout] and / or [B, Cout, H, W]; D3: rows of ycs floats and / or [B, Cout, Do, H, W]
    int M, K;
    int ntn;                                     // tiles along Cout (set by the launcher)
    // D3 only
    int D, Do, kd, padz;                         // stored depth, output depths (D, or 1: full-depth), depth taps, depth padding
    int pool;                                    // average each 2 x 2 (H, W) window: M counts the un-pooled positions, quad-major
    int ycs, yco;                                // y's row length and this conv's first channel in it
    int ntm, mfast;                              // tiles along M; mfast: consecutive tiles share their channels, not their positions
    // DL only (2-D, never with D3): its four values travel in the four depth words above, which no 2-D kernel reads, so the struct -- every
    // kernel's argument segment -- keeps its size and layout.  H, W are then the OUTPUT grid.
    __host__ __device__ void set_dl(int stride, int dilation, int pad, int bias_bs) { D = stride; Do = dilation; kd = pad; padz = bias_bs; }
    __device__ __forceinline__ int cstride() const { return D; }          // the conv's stride
    __device__ __forceinline__ int cdil() const { return Do; }            // its dilation
    __device__ __forceinline__ int cpad() const { return kd; }            // its zero padding
    __device__ __forceinline__ int bias_bs() const { return padz; }       // sample b adds bias[b bias_bs + n] (0: one bias for all)
};

__device__ __forceinline__ float leaky(float v, float slope) { return v < 0.0f ? slope * v : v; }
__device__ __forceinline__ float relu(float v) { return v < 0.0f ? 0.0f : v; }          // a NaN stays a NaN

// the position of a running k = ((kz ks + ky) ks + kx) Cin + ci
template <bool D3>
struct KPos {
    int ci, kx, ky, kz;
    __device__ __forceinline__ void init(int k, int Cin, int ks)
    {
        ci = k % Cin;
        int tap = k / Cin;
        kz = 0;
        if constexpr (D3) { kz = tap / (ks * ks); tap -= kz * ks * ks; }
        ky = tap / ks; kx = tap - ky * ks;
    }
    __device__ __forceinline__ void advance(int dk, int Cin, int ks)
    {
        ci += dk;
        while (ci >= Cin) {
            ci -= Cin;
            if (++kx == ks) {
                kx = 0; ++ky;
                if constexpr (D3) { if (ky == ks) { ky = 0; ++kz; } }
            }
        }
    }
};

// RP's part of a stage: slot j's prologue pair (its row's sample).  An empty base otherwise: the stage of every other kernel is the struct it was.
template <bool RP, int AV> struct StagePro { float4 rps4[AV], rpt4[AV]; };
template <int AV> struct StagePro<false, AV> {};

template <int PREC, bool VEC, bool D3, int WM, int WN, int TM, int TN, bool EXT = false, bool DL = false, bool RP = false>
__device__ __forceinline__ void conv_tile(const ConvArgs& g)
{
    static_assert(WM * WN == 4, "four waves");
    static_assert(!RP || (D3 && EXT && VEC && PREC == F32), "replicate padding with the per-sample prologue is the 3-D fp32 body, 16-byte loads");
    static_assert(!DL || (!D3 && PREC == F32), "the strided, dilated form is 2-D and fp32");
    static_assert(D3 || !EXT, "the extended epilogue belongs to the 3-D body");
    static_assert(PREC == F32 || PREC == BF16X3, "precision");
    constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
    constexpr int AV = BM / 32, WV = (BN + 31) / 32;           // VEC: float4 loads per thread (A, W)
    constexpr int AS = BM / 8, WS = BN / 8, KSTEP = 256 / BM;  // scalar: elements per thread; A's k stride between them
    typedef typename std::conditional<PREC == BF16X3, uint16_t, float>::type lds_t;      // BF16X3: rows of LDH bf16 (bf3_at)
    constexpr int LDR = PREC == BF16X3 ? LDH : LDK;
    __shared__ __attribute__((aligned(16))) lds_t As[2][BM * LDR];
    __shared__ __attribute__((aligned(16))) lds_t Ws[2][BN * LDR];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // Blocks are dealt to the 8 XCDs round-robin, and each XCD has an L2 of its own: block b takes tile (b % 8) (nblk / 8) + b / 8, so that
    // one XCD works on neighbouring pixel tiles (which share their taps' rows) and on all channel tiles of each (which share the taps).
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int tile = nblk % 8 == 0 ? (bid % 8) * (nblk / 8) + bid / 8 : bid;
    int m0 = (tile / g.ntn) * BM, n0 = (tile % g.ntn) * BN;
    if constexpr (D3) { if (g.mfast) { m0 = (tile % g.ntm) * BM; n0 = (tile / g.ntm) * BN; } }
    const int pad = DL ? g.cpad() : g.ks >> 1, hw = g.H * g.W;
    const int nsteps = (g.K + BK - 1) / BK;

    // ---- loader state ---------------------------------------------------------------------------------------------------------------
    // VEC: slot j is row (t >> 3) + 32 j of the tile, k entries 4 (t & 7) .. + 3 of the step (one tap, four channels);
    // scalar: row t % BM, k entries t / BM + KSTEP j (consecutive lanes read consecutive pixels: coalesced for an NCHW input)
    constexpr int NR = VEC ? AV : 1;
    int roy[NR], rox[NR], roz[D3 ? NR : 1]; size_t rbase[NR];   // a row's position (oy < 0: no such row) and its sample's offset
    int rpro[RP ? NR : 1];                                      // RP: the offset of the row's sample in ps and pt
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int m = m0 + (VEC ? (t >> 3) + 32 * j : t % BM);
        if constexpr (D3) roz[j] = 0;
        if (m < g.M) {
            if constexpr (D3) {
                int plane;
                if (g.pool) {
                    const int q = m >> 2, w2 = g.W >> 1, h2 = g.H >> 1, tq = q / w2, px = q - tq * w2;
                    plane = tq / h2;
                    roy[j] = 2 * (tq - plane * h2) + ((m >> 1) & 1); rox[j] = 2 * px + (m & 1);
                } else {
                    plane = m / hw;
                    const int r = m - plane * hw;
                    roy[j] = r / g.W; rox[j] = r - roy[j] * g.W;
                }
                const int b = plane / g.Do;
                roz[j] = plane - b * g.Do;
                rbase[j] = (size_t)b * g.D * g.Hs * g.Ws * g.Cin;
                if constexpr (RP) rpro[j] = b * g.Cin;
            } else {
                const int b = m / hw, r = m - b * hw;
                roy[j] = r / g.W; rox[j] = r - roy[j] * g.W;
                rbase[j] = (size_t)b * g.Hs * g.Ws * g.Cin;
            }
        } else { roy[j] = -1000000; rox[j] = 0; rbase[j] = 0; if constexpr (RP) rpro[j] = 0; }
    }
    KPos<D3> kp;
    kp.init(VEC ? 4 * (t & 7) : t / BM, g.Cin, g.ks);
    int kcur = VEC ? 4 * (t & 7) : t / BM;                      // the k of kp

    const int wm = (wave / WN) * TM * 16, wn = (wave % WN) * TN * 16;
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // the registers of one k step in flight between its global loads and its LDS stores
    struct Stage : StagePro<RP, VEC ? AV : 1> {
        float4 av4[VEC ? AV : 1], wv4[VEC ? WV : 1], ps4, pt4;
        float avs[VEC ? 1 : AS], wvs[VEC ? 1 : WS], pss[VEC ? 1 : AS], pts[VEC ? 1 : AS];
        unsigned inside;                                        // bit j: slot / element j came from inside the image
    };
    int knext = 0;                                              // the step the next load() fetches (steps are loaded in order)

    // the offset of tap (kz, ky, kx) of row slot j inside its sample, in pixels; false outside the (padded) volume
    auto tap = [&](int j, size_t& pix) -> bool {
        if constexpr (DL) {
            const int iy = roy[j] * g.cstride() - pad + kp.ky * g.cdil(), ix = rox[j] * g.cstride() - pad + kp.kx * g.cdil();
            if (!(iy >= 0 && iy < g.Hs && ix >= 0 && ix < g.Ws)) return false;
            pix = (size_t)iy * g.Ws + ix;
            return true;
        }
        if constexpr (RP) {
            if (roy[j] < 0) return false;                       // no such row; every tap of a row that exists is clamped into the volume
            const int iy = min(max(roy[j] - pad + kp.ky, 0), g.H - 1), ix = min(max(rox[j] - pad + kp.kx, 0), g.W - 1);
            const int iz = min(max(roz[j] - g.padz + kp.kz, 0), g.D - 1);
            pix = ((size_t)iz * g.Hs + iy) * g.Ws + ix;
            return true;
        }
        const int iy = roy[j] - pad + kp.ky, ix = rox[j] - pad + kp.kx;
        if (!(iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)) return false;
        pix = (size_t)(iy >> g.up) * g.Ws + (ix >> g.up);
        if constexpr (D3) {
            const int iz = roz[j] - g.padz + kp.kz;
            if (!(iz >= 0 && iz < g.D)) return false;
            pix += (size_t)iz * g.Hs * g.Ws;
        }
        return true;
    };

    auto load = [&](Stage& r) {
        r.inside = 0;
        if (knext >= nsteps) return;
        const int k0 = knext * BK;
        ++knext;
        if constexpr (VEC) {
            const bool kin = kcur < g.K;
#pragma unroll
            for (int j = 0; j < AV; ++j) {
                size_t pix;
                r.av4[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (kin && tap(j, pix)) {
                    r.av4[j] = *reinterpret_cast<const float4*>(g.x + rbase[j] + pix * g.Cin + kp.ci);
                    r.inside |= 1u << j;
                    if constexpr (RP) {
                        if (g.ps) {
                            r.rps4[j] = *reinterpret_cast<const float4*>(g.ps + rpro[j] + kp.ci);
                            r.rpt4[j] = *reinterpret_cast<const float4*>(g.pt + rpro[j] + kp.ci);
                        }
                    }
                }
            }
            if constexpr (!RP) {
                if (g.ps && kin) {
                    r.ps4 = *reinterpret_cast<const float4*>(g.ps + kp.ci);
                    r.pt4 = *reinterpret_cast<const float4*>(g.pt + kp.ci);
                }
            }
#pragma unroll
            for (int j = 0; j < WV; ++j) {
                const int row = (t >> 3) + 32 * j, n = n0 + row;
                r.wv4[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (row < BN && n < g.Cout && kin) r.wv4[j] = *reinterpret_cast<const float4*>(g.w + (size_t)n * g.K + kcur);
            }
            kp.advance(BK, g.Cin, g.ks);
            kcur += BK;
        } else {
#pragma unroll
            for (int j = 0; j < AS; ++j) {
                size_t pix;
                r.avs[j] = 0.0f; r.pss[j] = 1.0f; r.pts[j] = 0.0f;
                if (kcur < g.K && tap(0, pix)) {
                    const size_t off = g.in_nchw ? rbase[0] + (size_t)kp.ci * g.Hs * g.Ws + pix : rbase[0] + pix * g.Cin + kp.ci;
                    r.avs[j] = g.x[off];
                    if (g.ps) { r.pss[j] = g.ps[kp.ci]; r.pts[j] = g.pt[kp.ci]; }
                    r.inside |= 1u << j;
                }
                kp.advance(KSTEP, g.Cin, g.ks);
                kcur += KSTEP;
            }
#pragma unroll
            for (int j = 0; j < WS; ++j) {
                const int e = t + 256 * j, n = n0 + (e >> 5), k = k0 + (e & 31);
                r.wvs[j] = (n < g.Cout && k < g.K) ? g.w[(size_t)n * g.K + k] : 0.0f;
            }
        }
    };
    // BF16X3: a staged value goes to LDS as its three pieces (after the prologue and the zero outside the image)
    auto put4 = [&](lds_t* T, int row, const float4& v) {       // k entries 4 (t & 7) .. + 3 of the step
        if constexpr (PREC == BF16X3) {
            uint2 h, m, l;
            split_bf16x3(v, h, m, l);
            *reinterpret_cast<uint2*>(&T[bf3_at(row, 0, 4 * (t & 7))]) = h;
            *reinterpret_cast<uint2*>(&T[bf3_at(row, 1, 4 * (t & 7))]) = m;
            *reinterpret_cast<uint2*>(&T[bf3_at(row, 2, 4 * (t & 7))]) = l;
        } else {
            *reinterpret_cast<float4*>(&T[row * LDK + 4 * (t & 7)]) = v;
        }
    };
    auto put1 = [&](lds_t* T, int row, int k, float v) {
        if constexpr (PREC == BF16X3) split_bf16x3(v, T[bf3_at(row, 0, k)], T[bf3_at(row, 1, k)], T[bf3_at(row, 2, k)]);
        else T[row * LDK + k] = v;
    };
    auto store = [&](const Stage& r, int buf) {
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < AV; ++j) {
                float4 v = r.av4[j];
                if constexpr (RP) {
                    if (g.ps && (r.inside >> j & 1)) {
                        const float4 s4 = r.rps4[j], t4 = r.rpt4[j];
                        v.x = relu(fmaf(s4.x, v.x, t4.x)); v.y = relu(fmaf(s4.y, v.y, t4.y));
                        v.z = relu(fmaf(s4.z, v.z, t4.z)); v.w = relu(fmaf(s4.w, v.w, t4.w));
                    }
                } else if (g.ps && (r.inside >> j & 1)) {
                    v.x = leaky(fmaf(r.ps4.x, v.x, r.pt4.x), g.pslope); v.y = leaky(fmaf(r.ps4.y, v.y, r.pt4.y), g.pslope);
                    v.z = leaky(fmaf(r.ps4.z, v.z, r.pt4.z), g.pslope); v.w = leaky(fmaf(r.ps4.w, v.w, r.pt4.w), g.pslope);
                }
                put4(As[buf], (t >> 3) + 32 * j, v);
            }
#pragma unroll
            for (int j = 0; j < WV; ++j) {
                const int row = (t >> 3) + 32 * j;
                if (row < BN) put4(Ws[buf], row, r.wv4[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < AS; ++j) {
                float v = r.avs[j];
                if (g.ps && (r.inside >> j & 1)) v = leaky(fmaf(r.pss[j], v, r.pts[j]), g.pslope);
                put1(As[buf], t % BM, t / BM + KSTEP * j, v);
            }
#pragma unroll
            for (int j = 0; j < WS; ++j) { const int e = t + 256 * j; put1(Ws[buf], e >> 5, e & 31, r.wvs[j]); }
        }
    };
    // one k step of the block's tile out of LDS buffer `cur`
    auto compute = [&](int cur) {
        if constexpr (PREC == BF16X3) {
            // lane group lane >> 4 owns the same k entries 8 (lane >> 4) .. + 7, all eight in one MFMA: a piece's fragment is one 16-byte read
            bf16x8 a[TM][3], b[TN][3];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int p = 0; p < 3; ++p) a[i][p] = *reinterpret_cast<const bf16x8*>(&As[cur][bf3_at(wm + i * 16 + (lane & 15), p, 8 * (lane >> 4))]);
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int p = 0; p < 3; ++p) b[j][p] = *reinterpret_cast<const bf16x8*>(&Ws[cur][bf3_at(wn + j * 16 + (lane & 15), p, 8 * (lane >> 4))]);
            // the six products, smallest first: (activation piece, weight piece) = l.h, h.l, m.m, m.h, h.m, h.h
            constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PW[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
            for (int q = 0; q < 6; ++q)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][PA[q]], b[j][PW[q]], acc[i][j], 0, 0, 0);
        } else {
            // lane group lane >> 4 owns k entries 8 (lane >> 4) .. + 7 of the step, one per MFMA: the order of the sum is fixed, whichever
            float a[TM][8], b[TN][8];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const float* p = &As[cur][(wm + i * 16 + (lane & 15)) * LDK + 8 * (lane >> 4)];
                const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
                a[i][0] = lo.x; a[i][1] = lo.y; a[i][2] = lo.z; a[i][3] = lo.w; a[i][4] = hi.x; a[i][5] = hi.y; a[i][6] = hi.z; a[i][7] = hi.w;
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float* p = &Ws[cur][(wn + j * 16 + (lane & 15)) * LDK + 8 * (lane >> 4)];
                const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
                b[j][0] = lo.x; b[j][1] = lo.y; b[j][2] = lo.z; b[j][3] = lo.w; b[j][4] = hi.x; b[j][5] = hi.y; b[j][6] = hi.z; b[j][7] = hi.w;
            }
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][kk], b[j][kk], acc[i][j], 0, 0, 0);
        }
    };

    // Two register stages and two LDS buffers: step s is computed out of buffer s & 1 while step s + 1 (loaded one iteration earlier)
    // goes from its stage into the other buffer and step s + 3 leaves for that stage, so a load has two compute phases to arrive.
    Stage r0, r1;
    load(r0);                       // step 0
    store(r0, 0);
    load(r0);                       // step 1
    load(r1);                       // step 2
    __syncthreads();
    for (int s = 0; s < nsteps; s += 2) {
        compute(0);
        if (s + 1 < nsteps) store(r0, 1);
        load(r0);                   // step s + 3
        __syncthreads();
        if (s + 1 >= nsteps) break;
        compute(1);
        if (s + 2 < nsteps) store(r1, 0);
        load(r1);                   // step s + 4
        __syncthreads();
    }

    // D layout of 16x16x4: column lane & 15, rows 4 (lane >> 4) + r.  The bias and the residuals are fetched before they are needed.
    if constexpr (DL) {
        // every row's sample has a bias of its own, and the residual goes in before the ReLU
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + i * 16 + (lane >> 4) * 4 + r;
                if (m >= g.M) continue;
                const size_t brow = (size_t)(m / hw) * g.bias_bs();
                float bias[TN], res[TN];          // fetched before they are needed (res may alias y: read, then written, by this lane)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = n0 + wn + j * 16 + (lane & 15);
                    bias[j] = (g.bias && n < g.Cout) ? g.bias[brow + n] : 0.0f;
                    res[j] = (g.res && n < g.Cout) ? g.res[(size_t)m * g.Cout + n] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = n0 + wn + j * 16 + (lane & 15);
                    if (n >= g.Cout) continue;
                    float v = acc[i][j][r] + bias[j];
                    if (g.res) v += res[j];
                    if (g.act && v < 0.0f) v = 0.0f;
                    g.y[(size_t)m * g.ycs + g.yco + n] = v;
                }
            }
        return;
    }
    float bias[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn + j * 16 + (lane & 15);
        bias[j] = (g.bias && n < g.Cout) ? g.bias[n] : 0.0f;
    }
    if constexpr (D3) {
        auto activate = [&](float v) {
            if (g.act == 1) v = leaky(v, g.slope);
            else if (g.act == 2) v = 1.0f / (1.0f + expf(-v));
            return v;
        };
        float res[EXT ? TM : 1][4][EXT ? TN : 1];
        if constexpr (EXT) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const int m = m0 + wm + i * 16 + (lane >> 4) * 4 + r, n = n0 + wn + j * 16 + (lane & 15);
                        res[i][r][j] = (g.res && m < g.M && n < g.Cout) ? g.res[(size_t)m * g.Cout + n] : 0.0f;
                    }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int mq = m0 + wm + i * 16 + (lane >> 4) * 4;          // the lane's four rows mq .. mq + 3: one pooling window
            if (mq >= g.M) continue;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn + j * 16 + (lane & 15);
                if (n >= g.Cout) continue;
                if (g.pool) {                                           // M % 4 == 0: the window is whole
                    const float v0 = activate(acc[i][j][0] + bias[j]), v1 = activate(acc[i][j][1] + bias[j]);
                    const float v2 = activate(acc[i][j][2] + bias[j]), v3 = activate(acc[i][j][3] + bias[j]);
                    g.y[(size_t)(mq >> 2) * g.ycs + g.yco + n] = 0.25f * ((v0 + v1) + (v2 + v3));
                    continue;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = mq + r;
                    if (m >= g.M) continue;
                    float v = activate(acc[i][j][r] + bias[j]);
                    if constexpr (EXT) {
                        v += res[i][r][j];
                        if (g.split > 1) {                              // D = Do = 1: m = b hw + px
                            const int C = g.Cout / g.split, d = n / C, b = m / hw;
                            g.y[(((size_t)b * g.split + d) * hw + (m - b * hw)) * C + (n - d * C)] = v;
                            continue;
                        }
                    }
                    if (g.y) g.y[(size_t)m * g.ycs + g.yco + n] = v;
                    if (g.y_nchw) {
                        const int plane = m / hw, px = m - plane * hw, b = plane / g.Do, d = plane - b * g.Do;
                        g.y_nchw[(((size_t)b * g.Cout + n) * g.Do + d) * hw + px] = v;
                    }
                }
            }
        }
    } else {
        float res[TM][4][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int m = m0 + wm + i * 16 + (lane >> 4) * 4 + r, n = n0 + wn + j * 16 + (lane & 15);
                    res[i][r][j] = (g.res && m < g.M && n < g.Cout) ? g.res[(size_t)m * g.Cout + n] : 0.0f;
                }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + i * 16 + (lane >> 4) * 4 + r;
                if (m >= g.M) continue;
                const int b = m / hw, px = m - b * hw;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = n0 + wn + j * 16 + (lane & 15);
                    if (n >= g.Cout) continue;
                    float v = acc[i][j][r] + bias[j];
                    if (g.act == 1) v = leaky(v, g.slope);
                    else if (g.act == 2) v = 1.0f / (1.0f + expf(-v));
                    v += res[i][r][j];
                    if (g.y) g.y[(size_t)m * g.Cout + n] = v;
                    if (g.y_nchw) g.y_nchw[((size_t)b * g.Cout + n) * hw + px] = v;
                }
            }
    }
}

}  // namespace tconv
}  // namespace r3d
