// Z-buffer mesh rasteriser: MeshRenderer.forward of deep_3drecon/util/mesh_renderer.py:53-130 as SECC_Renderer configures it
// (pytorch3d's rasterize_meshes with image_size = S, blur_radius = 0, faces_per_pixel = 1, cull_backfaces = False under
// FoVPerspectiveCameras(fov, znear, zfar), identity pose, aspect 1), inference only, fp32.  The rule, restated from
// pytorch3d's naive rasteriser (tests/raster_ref64.py is its fp64 restatement; nothing here has been run against pytorch3d):
//   projection   x_ndc = s x / z, y_ndc = s y / z with s = 1 / tan(fov / 2); depth stays the camera-space z
//   pixel (i, j) y_ndc = -1 + (2 (S - 1 - i) + 1) / S, x_ndc = -1 + (2 (S - 1 - j) + 1) / S: +x is left, +y is up
//   face         edge(p, a, b) = (p.x - a.x)(b.y - a.y) - (p.y - a.y)(b.x - a.x); area = edge(v2, v0, v1), skipped when |area| <= 1e-8;
//                A = area + 1e-8; w0 = edge(p, v1, v2) / A, w1 = edge(p, v2, v0) / A, w2 = edge(p, v0, v1) / A; covered iff all three > 0;
//                t0 = w0 z1 z2, t1 = z0 w1 z2, t2 = z0 z1 w2, b_k = t_k / max(t0 + t1 + t2, 1e-8); pz = b0 z0 + b1 z1 + b2 z2, kept if >= 0
//   depth test   the smallest pz, the lower face index on an exact tie
//   near faces   a face with a vertex at z < znear / 2 (or z <= 0), a non-finite vertex or projection, or an index outside [0, N) is DROPPED
//                (pytorch3d clips the faces that cross z = znear / 2): no such face is ever read out of bounds or drawn.
// Three kernels behind one async memset of the key buffer to all ones:
//   scatter      one lane per (mesh, face): project, clamp the bounding box of the pixel centres to the image and walk it; every covered
//                pixel takes ONE 64-bit global atomic min of (bits(pz) << 32) | f.  A non-negative float orders as its bit pattern, so
//                the minimum is the nearest face and the lowest index on a tie whatever the order of execution: the result is
//                deterministic.  A face whose clamped box holds more than `large_box` pixels is appended to a list instead.
//   large_faces  a fixed grid of waves over that list (its length is read from device memory: no host sync): one wave per face, the lanes
//                striding the box.
//   resolve      one lane per pixel: the winning face from the key, pz from the key's upper half (the very value that won), the
//                barycentrics recomputed by the same device function, 3 C attributes gathered, pix_to_face / mask / depth / image written.
// Keys lie in tiles of 4 x 2 pixels = 64 bytes: an atomic leaves the L2 as 64-byte requests executed at the memory side, and a face of
// a few pixels then touches one or two of them, not one per image row.
#include "r3d_common.h"

namespace r3d {
namespace raster {

constexpr float EPS = 1e-8f;
constexpr int LARGE_BOX = 64;             // pixels in a clamped box above which a face goes to large_faces: what one wave covers in one stride
constexpr int LARGE_BLOCKS = 512;         // large_faces' fixed grid: 2048 waves
constexpr size_t COUNT_BYTES = 256;       // the list length's own 256 bytes between the keys and the list
constexpr unsigned long long EMPTY = ~0ull;

struct Args {
    const float* vertex;                  // [B, N, 3]
    const float* feat;                    // [B, N, C] or NULL
    const int* tri;                       // [M, 3] or [B, M, 3]
    int tri_batched, B, N, M, C, S;
    float s, zmin, xsign;                 // 1 / tan(fov / 2); znear / 2; -1 when x is negated
    int first_bg;
    float out_scale, out_shift;
    long long* pix_to_face;               // [B, S, S] or NULL
    float* mask;                          // [B, 1, S, S]
    float* depth;                         // [B, 1, S, S]
    float* image;                         // [B, C, S, S] or NULL
    unsigned long long* keys;             // [B, tiles_y, tiles_x, 2, 4]
    unsigned* count;                      // list length - 1 (all ones: empty), so that one memset clears keys and list
    unsigned* list;                       // [B M] packed indices b M + f
    int large_box, tiles_x;
    size_t keys_per_image;
};

struct Face { float x0, y0, x1, y1, x2, y2, z0, z1, z2, A; int i0, i1, i2; };

__device__ __forceinline__ float edge(float px, float py, float ax, float ay, float bx, float by)
{
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

__device__ __forceinline__ bool finite3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// the projected face (b, f), or false for a face that is dropped or skipped (header comment)
__device__ __forceinline__ bool load_face(const Args& a, int b, int f, Face& F)
{
    const int* t = a.tri + ((size_t)(a.tri_batched ? b : 0) * a.M + f) * 3;
    F.i0 = t[0]; F.i1 = t[1]; F.i2 = t[2];
    if ((unsigned)F.i0 >= (unsigned)a.N || (unsigned)F.i1 >= (unsigned)a.N || (unsigned)F.i2 >= (unsigned)a.N) return false;
    const float* V = a.vertex + (size_t)b * a.N * 3;
    const float* p0 = V + (size_t)F.i0 * 3;
    const float* p1 = V + (size_t)F.i1 * 3;
    const float* p2 = V + (size_t)F.i2 * 3;
    F.z0 = p0[2]; F.z1 = p1[2]; F.z2 = p2[2];
    if (!(F.z0 >= a.zmin && F.z1 >= a.zmin && F.z2 >= a.zmin && F.z0 > 0.0f && F.z1 > 0.0f && F.z2 > 0.0f)) return false;      // NaN fails too
    F.x0 = (a.s * (a.xsign * p0[0])) / F.z0; F.y0 = (a.s * p0[1]) / F.z0;
    F.x1 = (a.s * (a.xsign * p1[0])) / F.z1; F.y1 = (a.s * p1[1]) / F.z1;
    F.x2 = (a.s * (a.xsign * p2[0])) / F.z2; F.y2 = (a.s * p2[1]) / F.z2;
    if (!finite3(F.z0, F.z1, F.z2) || !finite3(F.x0, F.x1, F.x2) || !finite3(F.y0, F.y1, F.y2)) return false;
    const float area = edge(F.x2, F.y2, F.x0, F.y0, F.x1, F.y1);
    if (!(fabsf(area) > EPS)) return false;
    F.A = area + EPS;
    return true;
}

__device__ __forceinline__ float pixel_ndc(int i, int S) { return -1.0f + (float)(2 * (S - 1 - i) + 1) / (float)S; }

// the pixels whose centre can lie strictly between the NDC bounds lo < hi: pixel i sits at position S - 1/2 - (v + 1) S / 2 of that axis;
// 1/100 of a pixel covers the rounding of that expression for every S the entry point accepts (it costs no pixel: the coverage test decides)
__device__ __forceinline__ void pixel_range(float lo, float hi, int S, int& first, int& last)
{
    const float h = 0.5f * (float)S, top = (float)S - 0.5f;
    const float pf = fminf(fmaxf(top - (hi + 1.0f) * h - 0.01f, -1.0f), (float)S);
    const float pl = fminf(fmaxf(top - (lo + 1.0f) * h + 0.01f, -1.0f), (float)S);
    first = max((int)ceilf(pf), 0);
    last = min((int)floorf(pl), S - 1);
}

__device__ __forceinline__ void face_box(const Face& F, int S, int& x0, int& x1, int& y0, int& y1)
{
    pixel_range(fminf(fminf(F.x0, F.x1), F.x2), fmaxf(fmaxf(F.x0, F.x1), F.x2), S, x0, x1);
    pixel_range(fminf(fminf(F.y0, F.y1), F.y2), fmaxf(fmaxf(F.y0, F.y1), F.y2), S, y0, y1);
}

// rule 4 at the pixel centre (px, py): covered, and the perspective-corrected barycentrics and depth (meaningful when covered)
__device__ __forceinline__ bool eval(const Face& F, float px, float py, float& b0, float& b1, float& b2, float& pz)
{
    const float w0 = edge(px, py, F.x1, F.y1, F.x2, F.y2) / F.A;
    const float w1 = edge(px, py, F.x2, F.y2, F.x0, F.y0) / F.A;
    const float w2 = edge(px, py, F.x0, F.y0, F.x1, F.y1) / F.A;
    const float t0 = w0 * F.z1 * F.z2, t1 = F.z0 * w1 * F.z2, t2 = F.z0 * F.z1 * w2;
    const float den = fmaxf(t0 + t1 + t2, EPS);
    b0 = t0 / den; b1 = t1 / den; b2 = t2 / den;
    pz = b0 * F.z0 + b1 * F.z1 + b2 * F.z2;
    return w0 > 0.0f && w1 > 0.0f && w2 > 0.0f;
}

__device__ __forceinline__ size_t key_index(const Args& a, int b, int y, int x)
{
    return (size_t)b * a.keys_per_image + ((size_t)(y >> 1) * a.tiles_x + (x >> 2)) * 8 + (y & 1) * 4 + (x & 3);
}

__device__ __forceinline__ void draw(const Args& a, const Face& F, int b, int f, int y, int x)
{
    float b0, b1, b2, pz;
    if (eval(F, pixel_ndc(x, a.S), pixel_ndc(y, a.S), b0, b1, b2, pz) && pz >= 0.0f)
        atomicMin(a.keys + key_index(a, b, y, x), ((unsigned long long)__float_as_uint(pz) << 32) | (unsigned)f);
}

__global__ void __launch_bounds__(256) scatter(Args a)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (size_t)a.B * a.M) return;
    const int b = (int)(g / a.M), f = (int)(g - (size_t)b * a.M);
    Face F;
    if (!load_face(a, b, f, F)) return;
    int x0, x1, y0, y1;
    face_box(F, a.S, x0, x1, y0, y1);
    if (x1 < x0 || y1 < y0) return;
    if ((long long)(x1 - x0 + 1) * (y1 - y0 + 1) > a.large_box) {
        const unsigned slot = atomicAdd(a.count, 1u) + 1u;          // the counter starts at all ones: the first slot is 0
        if (slot < (size_t)a.B * a.M) a.list[slot] = (unsigned)g;     // always true after the call's clear; a stage run without one must not write past the list
        return;
    }
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) draw(a, F, b, f, y, x);
}

__global__ void __launch_bounds__(256) large_faces(Args a)
{
    const unsigned total = (unsigned)((size_t)a.B * a.M);
    const unsigned n = min(*a.count + 1u, total);
    const unsigned waves = gridDim.x * 4, wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (unsigned e = wave; e < n; e += waves) {
        const unsigned g = a.list[e];
        if (g >= total) continue;
        const int b = (int)(g / (unsigned)a.M), f = (int)(g - (unsigned)b * (unsigned)a.M);
        Face F;
        if (!load_face(a, b, f, F)) continue;
        int x0, x1, y0, y1;
        face_box(F, a.S, x0, x1, y0, y1);
        if (x1 < x0 || y1 < y0) continue;
        const int w = x1 - x0 + 1;
        const long long px = (long long)w * (y1 - y0 + 1);
        for (long long i = lane; i < px; i += 64) {
            const int dy = (int)(i / w);
            draw(a, F, b, f, y0 + dy, x0 + (int)(i - (long long)dy * w));
        }
    }
}

__global__ void __launch_bounds__(256) resolve(Args a)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, hw = (size_t)a.S * a.S;
    if (g >= (size_t)a.B * hw) return;
    const int b = (int)(g / hw);
    const size_t p = g - (size_t)b * hw;
    const int y = (int)(p / a.S), x = (int)(p - (size_t)y * a.S);
    const unsigned long long key = a.keys[key_index(a, b, y, x)];
    Face F;
    int f = -1;
    if (key != EMPTY) {
        f = (int)(unsigned)(key & 0xffffffffull);
        if ((unsigned)f >= (unsigned)a.M || !load_face(a, b, f, F)) f = -1;          // cannot happen after scatter; never read out of bounds
    }
    const long long packed = f < 0 ? -1 : (long long)b * a.M + f;
    // mask = pix_to_face > 0 (mesh_renderer.py:116): the first face of the batch's first mesh is background; >= 0 when asked
    const float m = (packed > 0 || (packed == 0 && !a.first_bg)) ? 1.0f : 0.0f;
    if (a.pix_to_face) a.pix_to_face[g] = packed;
    a.mask[g] = m;
    a.depth[g] = f < 0 ? 0.0f : m * __uint_as_float((unsigned)(key >> 32));
    if (!a.image) return;
    float* out = a.image + (size_t)b * a.C * hw + p;
    if (f < 0) {
        for (int c = 0; c < a.C; ++c) out[(size_t)c * hw] = a.out_shift;
        return;
    }
    float b0, b1, b2, pz;
    eval(F, pixel_ndc(x, a.S), pixel_ndc(y, a.S), b0, b1, b2, pz);
    const float* A = a.feat + (size_t)b * a.N * a.C;
    const float* f0 = A + (size_t)F.i0 * a.C;
    const float* f1 = A + (size_t)F.i1 * a.C;
    const float* f2 = A + (size_t)F.i2 * a.C;
    for (int c = 0; c < a.C; ++c) out[(size_t)c * hw] = (m * (b0 * f0[c] + b1 * f1[c] + b2 * f2[c])) * a.out_scale + a.out_shift;
}

inline size_t keys_per_image(int S) { return (size_t)((S + 3) / 4) * ((S + 1) / 2) * 8; }

// the sizes every entry point accepts: B, N, M >= 1, 1 <= S <= 16384 (a pixel centre's numerator is exact in fp32), C in 1 .. 4, B M and B S S
// below 2^31.  With a name the first miss is that entry point's message; without one (r3d_raster_workspace_bytes, which knows neither N
// nor C and passes 1 for both) nothing is said.
static bool sizes_ok(const char* what, int B, int N, int M, int C, int S)
{
    auto no = [&](const char* fmt, auto... v) { if (what) set_error(fmt, what, v...); return false; };
    if (S < 1 || S > 16384) return no("%s: image size S = %d is not in 1 .. 16384", S);
    if (B < 1 || N < 1 || M < 1) return no("%s: bad argument (B = %d, N = %d, M = %d must be positive)", B, N, M);
    if (C < 1 || C > 4) return no("%s: C = %d attribute channels, supported are 1 .. 4", C);
    return below_2_31(what, "B M", (double)B * M, "faces (the packed 31-bit face index)") && below_2_31(what, "B S S", (double)B * S * S, "pixels");
}

inline size_t workspace_bytes(int B, int S, int M)
{
    return (size_t)B * keys_per_image(S) * 8 + COUNT_BYTES + (((size_t)B * M * 4 + 255) & ~(size_t)255);
}

enum { STAGE_CLEAR = 1, STAGE_SCATTER = 2, STAGE_LARGE = 4, STAGE_RESOLVE = 8, STAGE_ALL = 15 };

static int forward(const float* vertex, const float* feat, const int32_t* tri, int tri_batched, int B, int N, int M, int C, int S,
                   float fov_deg, float znear, int negate_x, int first_face_is_background, float out_scale, float out_shift,
                   int64_t* pix_to_face, float* mask, float* depth, float* image, void* workspace, size_t workspace_bytes_given,
                   int large_box, int stages, hipStream_t st)
{
    if (!vertex || !tri || !mask || !depth) { set_error("raster_forward: NULL pointer (vertex, tri, mask and depth are required)"); return R3D_ERR_INVALID_ARG; }
    if ((feat == nullptr) != (image == nullptr)) { set_error("raster_forward: feat and image are given together or not at all"); return R3D_ERR_INVALID_ARG; }
    if (!sizes_ok("raster_forward", B, N, M, feat ? C : 1, S) || !below_2_31("raster_forward", "4 B N", 4.0 * B * N, "elements")) return R3D_ERR_INVALID_ARG;
    if (!(fov_deg > 0.0f && fov_deg < 180.0f)) { set_error("raster_forward: fov_deg = %g is not a finite angle in (0, 180)", (double)fov_deg); return R3D_ERR_INVALID_ARG; }
    if (!(znear == znear) || !(out_scale == out_scale) || !(out_shift == out_shift)) { set_error("raster_forward: znear or the output affine is NaN"); return R3D_ERR_INVALID_ARG; }
    if (large_box < 0 || stages < 0 || stages > STAGE_ALL) { set_error("raster_forward: bad test-hook argument"); return R3D_ERR_INVALID_ARG; }
    if (!workspace_ok("raster_forward", workspace, workspace_bytes_given, workspace_bytes(B, S, M), 8, "r3d_raster_workspace_bytes")) return R3D_ERR_WORKSPACE;

    Args a;
    a.vertex = vertex; a.feat = feat; a.tri = tri;
    a.tri_batched = tri_batched ? 1 : 0; a.B = B; a.N = N; a.M = M; a.C = feat ? C : 0; a.S = S;
    a.s = (float)(1.0 / tan((double)fov_deg * 0.5 * 3.14159265358979323846 / 180.0));
    a.zmin = 0.5f * znear; a.xsign = negate_x ? -1.0f : 1.0f;
    a.first_bg = first_face_is_background ? 1 : 0; a.out_scale = out_scale; a.out_shift = out_shift;
    a.pix_to_face = (long long*)pix_to_face; a.mask = mask; a.depth = depth; a.image = image;
    a.keys_per_image = keys_per_image(S);
    const size_t key_bytes = (size_t)B * a.keys_per_image * 8;
    a.keys = (unsigned long long*)workspace;
    a.count = (unsigned*)((char*)workspace + key_bytes);
    a.list = (unsigned*)((char*)workspace + key_bytes + COUNT_BYTES);
    a.large_box = large_box; a.tiles_x = (S + 3) / 4;

    ProfScope ps(R3D_PROF_MISC, st);
    if ((stages & STAGE_CLEAR) && hipMemsetAsync(workspace, 0xFF, key_bytes + COUNT_BYTES, st) != hipSuccess) return check_launch("raster_forward (clear)");
    const size_t faces = (size_t)B * M, pixels = (size_t)B * S * S;
    if (stages & STAGE_SCATTER) hipLaunchKernelGGL(scatter, dim3((unsigned)((faces + 255) / 256)), dim3(256), 0, st, a);
    if (stages & STAGE_LARGE) hipLaunchKernelGGL(large_faces, dim3(LARGE_BLOCKS), dim3(256), 0, st, a);
    if (stages & STAGE_RESOLVE) hipLaunchKernelGGL(resolve, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, st, a);
    return check_launch("raster_forward");
}

}  // namespace raster
}  // namespace r3d

using namespace r3d;

extern "C" size_t r3d_raster_workspace_bytes(int B, int S, int M)
{
    return raster::sizes_ok(nullptr, B, 1, M, 1, S) ? raster::workspace_bytes(B, S, M) : 0;
}

extern "C" int r3d_raster_forward(const float* vertex, const float* feat, const int32_t* tri, int tri_batched, int B, int N, int M, int C, int S,
                                  float fov_deg, float znear, int negate_x, int first_face_is_background, float out_scale, float out_shift,
                                  int64_t* pix_to_face, float* mask, float* depth, float* image, void* workspace, size_t workspace_bytes,
                                  r3d_stream_t stream)
{
    return raster::forward(vertex, feat, tri, tri_batched, B, N, M, C, S, fov_deg, znear, negate_x, first_face_is_background, out_scale, out_shift,
                           pix_to_face, mask, depth, image, workspace, workspace_bytes, raster::LARGE_BOX, raster::STAGE_ALL, (hipStream_t)stream);
}

// Test hook outside the C ABI of include/r3d_hip.h (OPTIONAL_SIGNATURES of real3dportrait_amd/_lib.py): the same call with the large-face
// threshold given (tests/test_gpu_raster.py sends one face down both paths) and only the stages of a bit mask run (1 clear, 2 scatter,
// 4 large_faces, 8 resolve: scripts/prof_raster.py times them one by one).
extern "C" int r3d_debug_raster_forward(const float* vertex, const float* feat, const int32_t* tri, int tri_batched, int B, int N, int M, int C,
                                        int S, float fov_deg, float znear, int negate_x, int first_face_is_background, float out_scale,
                                        float out_shift, int64_t* pix_to_face, float* mask, float* depth, float* image, void* workspace,
                                        size_t workspace_bytes, int large_box, int stages, r3d_stream_t stream)
{
    return raster::forward(vertex, feat, tri, tri_batched, B, N, M, C, S, fov_deg, znear, negate_x, first_face_is_background, out_scale, out_shift,
                           pix_to_face, mask, depth, image, workspace, workspace_bytes, large_box, stages, (hipStream_t)stream);
}
