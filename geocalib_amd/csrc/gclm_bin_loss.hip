// gclm_bin_loss.hip -- gclm_bin_loss / gclm_bin_loss_grad: the loss the classification heads are trained with, per image, and
// its gradient with respect to the logits -- per-pixel cross-entropy of the up logits (B, Ku, H, W) and the latitude logits
// (B, Kl, H, W) against the bins of a calibration's perspective fields (perspective_encoding.encode_up_bin /
// encode_bin_latitude of get_perspective_field), with the target evaluated per pixel in registers (gclm_render.h: persp_up
// normalised, persp_lat) instead of rendered, encoded and handed to a log_softmax the size of the logits.
//
// Per pixel of one head, with z its K logits (16-bit logits are the floats they widen to) and t its target bin:
//   lse = log sum_k exp z_k      ce = lse - z_t      hit = [argmax_k z_k == t]   (torch.argmax: the first of the greatest, NaN above all)
// Per image: numerator sum w ce, denominator sum w (w = the head's confidence; H W without one), hits = sum hit.
// The gradient of a pixel's logit k is scale[b, head] * w * (exp(z_k - lse) - [k == t]); the caller forms scale = grad_output *
// weight / denominator from the forward's d_out.  The forward leaves lse and the bins it used (B, 2, H, W) for the gradient
// call, which does NOT evaluate the target again: with -ffp-contract=fast a second evaluation in another kernel may round
// differently and move a boundary pixel to the neighbouring bin between the two passes.
//
// Target bins (float32, the reference's expressions):
//   up        degrees = atan2(t_y, t_x) 180 / pi + 180; bin = rint(degrees / (360 / (Ku - 1))), a full turn wraps to 0; a target
//             that is exactly (0, 0) is the invalid class Ku - 1
//   latitude  class k holds the degrees in (-90 + k 180 / Kl, -90 + (k + 1) 180 / Kl], the first and the last open-ended:
//             ceil((degrees + 90) Kl / 180) - 1 clamped to 0 .. Kl - 1
//
// Forward: the tile walk of gclm_render.h.  A lane holds PX adjacent pixels -- 4 float32 or 8 16-bit logits per 16-byte load
// where W and the planes allow it, else 1 -- and streams the K channel planes kBinsUnroll loads at a time, keeping per pixel the
// running maximum (which is also argmax's `best`), its first index and the sum of exp(z - maximum), rescaled once per GROUP of
// channels.  z_t is one more load per pixel, at the target's plane.
// The sums of a tile do not depend on PX: a lane's values are added in the tree the one-pixel walk adds them in -- a
// butterfly over the 64 pixels one wave of that walk holds (here 64 / PX lanes of PX pixels), the four rows in order -- and a
// tile leaves one record per 64-pixel column at the index the one-pixel walk gives it.  bin_loss_finish_kernel (grid = B) sums
// an image's records in float64 in eight chains.  No atomics: an image's bits depend on that image alone, not on the path.
// Gradient: the same walk, no reduction, no LDS; the logits are read once more and the gradient leaves in non-temporal stores
// in the logits' type, rounded to nearest even.  Offsets into the logits are size_t.  No scratch.
// Both paths give the same bits, per pixel and per image: the arithmetic on the logits is compiled without contraction.
#include "gclm_field_loss.h"
#include "gclm_logits.h"

namespace gclm {
namespace {

// Contraction is OFF for everything written in this file (the target formulas of gclm_render.h keep the build's setting): the
// arithmetic on the logits is compiled into a 16-byte and a one-pixel instantiation per logit type, which must agree bit for
// bit -- left to itself the compiler fuses (z - lse) log2(e) or w (p - 1) in one of them and not in the other.
// (Needs -ffp-contract=fast-honor-pragmas, the Makefile's; plain `fast` ignores the pragma.)
#pragma clang fp contract(off)

constexpr int kBinHeadWords = 3;                 // per head: sum w ce, sum w, hits
constexpr int kBinWords = 2 * kBinHeadWords;     // float sums per record: up, then latitude
constexpr int kBinChains = 8;                    // summation chains per image of the second launch
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kDegPerRad = 57.29577951308232f;

struct BinLossArgs {
    const float *cam, *grav;
    const void *upl, *latl;
    const float *upc, *latc;
    float *rec, *lse;
    int16_t* bins;
    int H, W, tiles_x, tiles_x1, Ku, Kl;         // tiles_x: tile columns of this walk; tiles_x1: of the one-pixel walk
};

struct BinLossGradArgs {
    const void *upl, *latl;
    const float *upc, *latc, *lse, *scale;
    const int16_t* bins;
    void *gup, *glat;
    int H, W, tiles_x, Ku, Kl;
};

__device__ __forceinline__ int encode_up(f32x2 t, int K) {
    if (t.x == 0.f && t.y == 0.f) return K - 1;
    const float degrees = atan2f(t.y, t.x) * kDegPerRad + 180.f;
    const int bin = (int)__builtin_rintf(degrees / (360.f / (float)(K - 1)));
    return bin >= K - 1 || bin < 0 ? 0 : bin;    // (whatever a NaN target converts to: a bin inside 0 .. K - 1, z_t is read there)
}

__device__ __forceinline__ int encode_lat(float lat, int K) {
    const int bin = (int)ceilf((lat * kDegPerRad + 90.f) * ((float)K / 180.f)) - 1;
    return bin < 0 ? 0 : (bin > K - 1 ? K - 1 : bin);
}

// v - m with an infinite m taken as 0, so that a pixel whose maximum is +-inf gets lse = +-inf instead of NaN
__device__ __forceinline__ float finite_or_zero(float m) { return fabsf(m) == __builtin_inff() ? 0.f : m; }
__device__ __forceinline__ float exp_of(float x) { return __builtin_amdgcn_exp2f(x * kLog2e); }

// PX floats / bins of a plane at pixel offset o (a multiple of PX where PX > 1, the plane 16-byte aligned)
template <int PX>
__device__ __forceinline__ void load_floats(const float* __restrict__ p, float (&v)[PX]) {
    if constexpr (PX == 1) v[0] = *p;
    else {
#pragma unroll
        for (int q = 0; q < PX / 4; ++q) {
            const f32x4 t = reinterpret_cast<const f32x4*>(p)[q];
            v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
        }
    }
}
template <int PX>
__device__ __forceinline__ void store_floats(const float (&v)[PX], float* __restrict__ p) {
    if constexpr (PX == 1) *p = v[0];
    else {
#pragma unroll
        for (int q = 0; q < PX / 4; ++q) reinterpret_cast<f32x4*>(p)[q] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
    }
}
typedef uint32_t bins_u2 __attribute__((ext_vector_type(2)));
template <int PX>
__device__ __forceinline__ void load_bins(const int16_t* __restrict__ p, int (&t)[PX]) {
    if constexpr (PX == 1) t[0] = *p;
    else {
        uint32_t w[PX / 2];
        if constexpr (PX == 4) {
            const bins_u2 q = *reinterpret_cast<const bins_u2*>(p);
            w[0] = q.x, w[1] = q.y;
        } else {
            const bins_u4 q = *reinterpret_cast<const bins_u4*>(p);
            w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) t[j] = (int)(int16_t)((j & 1) ? w[j >> 1] >> 16 : w[j >> 1] & 0xffffu);
    }
}
template <int PX>
__device__ __forceinline__ void store_bins(const int (&t)[PX], int16_t* __restrict__ p) {
    if constexpr (PX == 1) *p = (int16_t)t[0];
    else {
        uint32_t w[PX / 2];
#pragma unroll
        for (int j = 0; j < PX / 2; ++j) w[j] = ((uint32_t)t[2 * j] & 0xffffu) | ((uint32_t)t[2 * j + 1] << 16);
        if constexpr (PX == 4) *reinterpret_cast<bins_u2*>(p) = bins_u2{w[0], w[1]};
        else *reinterpret_cast<bins_u4*>(p) = bins_u4{w[0], w[1], w[2], w[3]};
    }
}

// The float32 gradient as a value of its own before it is narrowed: handed a product, the compiler narrows it in the
// multiply (v_fma_mixlo_f16: one rounding of the exact product) on the one-pixel path and converts the rounded float32
// (v_cvt_pk_f16_f32) on the 16-byte path -- a last-bit difference between the paths, and only the second is float32 .to(float16).
__device__ __forceinline__ float as_float32(float v) {
    asm volatile("" : "+v"(v));                  // (no instruction: the value just has to exist in a register)
    return v;
}

// The gradient's store: PX values narrowed to the logits' type, one non-temporal store (16 bytes where PX > 1).
template <int DT, int PX>
__device__ __forceinline__ void store_grad(bins_elem<DT>* __restrict__ plane, size_t i, const float (&v)[PX]) {
    if constexpr (PX == 1) {
        __builtin_nontemporal_store(pack_narrow<DT>(as_float32(v[0])), plane + i);
    } else {
        bins_u4 q;
        if constexpr (DT == GCLM_LOGITS_F32) {
            q = bins_u4{__builtin_bit_cast(uint32_t, v[0]), __builtin_bit_cast(uint32_t, v[1]), __builtin_bit_cast(uint32_t, v[2]),
                        __builtin_bit_cast(uint32_t, v[3])};
        } else {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                w[k] = (uint32_t)pack_narrow<DT>(as_float32(v[2 * k])) | ((uint32_t)pack_narrow<DT>(as_float32(v[2 * k + 1])) << 16);
            }
            q = bins_u4{w[0], w[1], w[2], w[3]};
        }
        __builtin_nontemporal_store(q, reinterpret_cast<bins_u4*>(plane) + i);
    }
}

// lse and argmax of the K logits of this lane's PX pixels: z is the first plane of the image's head, hw the planes' stride,
// i the lane's unit in a plane (its pixel offset / PX).  `best` is torch.argmax's running maximum (bins_argmax's rule in
// gclm_fields.hip: a later x replaces it only if it is no NaN and x <= best is false) and the maximum the sum is taken
// against; one group of N channels costs one rescale of the sum.
template <int DT, int PX>
__device__ __forceinline__ void head_lse(const bins_elem<DT>* __restrict__ z, int K, size_t hw, size_t i, float (&lse)[PX], int (&arg)[PX]) {
    float best[PX], s[PX], v[kBinsUnroll][PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) best[j] = -__builtin_inff(), s[j] = 0.f, arg[j] = 0;
    auto group = [&](int c, auto n) {
        constexpr int N = decltype(n)::value;
        float old[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) old[j] = best[j];
#pragma unroll
        for (int u = 0; u < N; ++u) {
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const bool t = !(v[u][j] <= best[j]) && best[j] == best[j];
                best[j] = t ? v[u][j] : best[j];
                arg[j] = t ? c + u : arg[j];
            }
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const float m = finite_or_zero(best[j]);
            float acc = 0.f;
#pragma unroll
            for (int u = 0; u < N; ++u) acc += exp_of(v[u][j] - m);
            // (nothing summed yet: the factor would be exp(-inf - m), or 0 inf where m is far below 0)
            const float f = old[j] == -__builtin_inff() ? 0.f : exp_of(finite_or_zero(old[j]) - m);
            s[j] = s[j] * f + acc;
        }
    };
    int c = 0;
    for (; c + kBinsUnroll <= K; c += kBinsUnroll) {
#pragma unroll
        for (int u = 0; u < kBinsUnroll; ++u) bins_load<DT, PX>(z + (size_t)(c + u) * hw, i, v[u]);
        group(c, std::integral_constant<int, kBinsUnroll>{});
    }
    for (; c < K; ++c) {                          // the remainder: groups of one
        bins_load<DT, PX>(z + (size_t)c * hw, i, v[0]);
        group(c, std::integral_constant<int, 1>{});
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) lse[j] = finite_or_zero(best[j]) + logf(s[j]);
}

// The sum of `v` over the 64 pixels that one wave of the one-pixel walk holds -- here the PX pixels of each of 64 / PX adjacent
// lanes -- in that walk's order: wave_sum's butterfly over pixel index e, e ^ 32 first, e ^ 1 last.  A pixel's index is
// PX (lane % (64 / PX)) + j, so the high steps cross lanes and the last log2(PX) ones stay inside a lane.  Every lane of the
// group ends with the same bits (a + b and b + a are the same float).
template <int PX>
__device__ __forceinline__ float group_sum(float (&v)[PX]) {
#pragma unroll
    for (int o = 32 / PX; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < PX; ++j) v[j] += __shfl_xor(v[j], o, 64);
    }
#pragma unroll
    for (int h = PX / 2; h > 0; h >>= 1) {
#pragma unroll
        for (int j = 0; j < h; ++j) v[j] += v[j + h];
    }
    return v[0];
}

// One head of the forward at this lane's pixels: writes lse and the bins, returns the group's three sums.
template <int DT, int PX>
__device__ __forceinline__ void head_forward(const void* logits, int K, const float* conf, size_t b, size_t hw, size_t o, bool in,
                                             const int (&t)[PX], float* lse_plane, int16_t* bin_plane, float (&sum)[kBinHeadWords]) {
    float wce[PX], w[PX], hit[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) wce[j] = 0.f, w[j] = 0.f, hit[j] = 0.f;
    if (in) {
        const bins_elem<DT>* z = static_cast<const bins_elem<DT>*>(logits) + b * (size_t)K * hw;
        float lse[PX];
        int arg[PX];
        head_lse<DT, PX>(z, K, hw, o / PX, lse, arg);
        if (conf) load_floats<PX>(conf + b * hw + o, w);
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            float zt[1];
            bins_load<DT, 1>(z + (size_t)t[j] * hw, o + j, zt);
            const float ce = lse[j] - zt[0];
            wce[j] = conf ? w[j] * ce : ce;
            hit[j] = arg[j] == t[j] ? 1.f : 0.f;
        }
        store_floats<PX>(lse, lse_plane + o);
        store_bins<PX>(t, bin_plane + o);
    }
    sum[0] = group_sum<PX>(wce);
    sum[1] = conf ? group_sum<PX>(w) : 0.f;       // (without a confidence the denominator is H W: the finish kernel's)
    sum[2] = group_sum<PX>(hit);
}

template <int MODEL, int DT, int PX>
__global__ __launch_bounds__(kBlock) void bin_loss_kernel(const BinLossArgs a) {
    __shared__ float s_sum[kTileRows][PX][kBinWords];
    int x, y;
    const bool in = tile_pixel<PX>(a.tiles_x, a.H, a.W, x, y);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t b = blockIdx.y, hw = (size_t)a.H * a.W, o = (size_t)y * a.W + x;
    int tu[PX], tl[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) tu[j] = 0, tl[j] = 0;
    if (in) {
        float u[PX], r2[PX];
        const PerspRow r = lane_row<PX>(a.cam, a.grav, (int)b, x, y, u, r2);
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            if (a.upl) tu[j] = encode_up(persp_up<MODEL>(r, u[j], r2[j], true), a.Ku);
            if (a.latl) tl[j] = encode_lat(persp_lat<MODEL>(r, u[j], r2[j]), a.Kl);
        }
    }
    float sum[2][kBinHeadWords] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    if (a.upl) head_forward<DT, PX>(a.upl, a.Ku, a.upc, b, hw, o, in, tu, a.lse + b * 2 * hw, a.bins + b * 2 * hw, sum[0]);
    if (a.latl) head_forward<DT, PX>(a.latl, a.Kl, a.latc, b, hw, o, in, tl, a.lse + (b * 2 + 1) * hw, a.bins + (b * 2 + 1) * hw, sum[1]);
    // every lane of the block from here on: one record per 64-pixel group and row in LDS, the four rows added in order, one
    // record per group in the workspace -- where the one-pixel walk has a tile
    constexpr int kGroupLanes = 64 / PX;
    if (lane % kGroupLanes == 0) {
#pragma unroll
        for (int k = 0; k < kBinWords; ++k) s_sum[wave][lane / kGroupLanes][k] = sum[k / kBinHeadWords][k % kBinHeadWords];
    }
    __syncthreads();
    const int g = threadIdx.x / kBinWords, k = threadIdx.x % kBinWords;
    const int ty = blockIdx.x / a.tiles_x, tx1 = (blockIdx.x - ty * a.tiles_x) * PX + g;
    if (g < PX && tx1 < a.tiles_x1) {
        float v = s_sum[0][g][k];
        for (int row = 1; row < kTileRows; ++row) v += s_sum[row][g][k];
        const size_t tiles1 = (size_t)a.tiles_x1 * (gridDim.x / a.tiles_x);
        a.rec[(b * tiles1 + (size_t)ty * a.tiles_x1 + tx1) * kBinWords + k] = v;
    }
}

// One block per image: word k of the image's records is summed by kBinChains chains (record t goes to chain t % kBinChains),
// the chains are added in order, all in float64.  out (B, 6) = [up numerator, denominator, hits, latitude numerator,
// denominator, hits]: the denominator is H W, or sum conf where that confidence is given; NaN for an absent head.
__global__ __launch_bounds__(kBlock) void bin_loss_finish_kernel(const float* __restrict__ rec, int tiles, int hw, int has_up, int has_upc,
                                                                 int has_lat, int has_latc, float* __restrict__ out) {
    __shared__ double part[kBinChains][kBinWords];
    const int b = blockIdx.x, k = threadIdx.x & 31, chain = threadIdx.x >> 5;
    if (k < kBinWords) part[chain][k] = chain_sum<kBinChains>(rec + (size_t)b * tiles * kBinWords + k, kBinWords, tiles, chain);
    __syncthreads();
    const int word = threadIdx.x;
    if (word < kBinWords) {
        const int head = word / kBinHeadWords;
        const bool has = head ? has_lat != 0 : has_up != 0, hasc = head ? has_latc != 0 : has_upc != 0;
        double v = column_sum(part, word);
        if (word % kBinHeadWords == 1 && !hasc) v = (double)hw;
        out[(size_t)b * kBinWords + word] = has ? (float)v : __builtin_nanf("");
    }
}

// One head of the gradient at this lane's pixels.
template <int DT, int PX>
__device__ __forceinline__ void head_grad(const void* logits, int K, const float* conf, float scale, size_t b, size_t hw, size_t o,
                                          const float* lse_plane, const int16_t* bin_plane, void* grad) {
    const bins_elem<DT>* z = static_cast<const bins_elem<DT>*>(logits) + b * (size_t)K * hw;
    bins_elem<DT>* g = static_cast<bins_elem<DT>*>(grad) + b * (size_t)K * hw;
    float lse[PX], w[PX], v[kBinsUnroll][PX];
    int t[PX];
    load_floats<PX>(lse_plane + o, lse);
    load_bins<PX>(bin_plane + o, t);
    if (conf) {
        load_floats<PX>(conf + b * hw + o, w);
#pragma unroll
        for (int j = 0; j < PX; ++j) w[j] *= scale;
    } else {
#pragma unroll
        for (int j = 0; j < PX; ++j) w[j] = scale;
    }
    const size_t i = o / PX;
    auto group = [&](int c, auto n) {
        constexpr int N = decltype(n)::value;
#pragma unroll
        for (int u = 0; u < N; ++u) {
#pragma unroll
            for (int j = 0; j < PX; ++j) v[u][j] = w[j] * (exp_of(v[u][j] - lse[j]) - (c + u == t[j] ? 1.f : 0.f));
            store_grad<DT, PX>(g + (size_t)(c + u) * hw, i, v[u]);
        }
    };
    int c = 0;
    for (; c + kBinsUnroll <= K; c += kBinsUnroll) {
#pragma unroll
        for (int u = 0; u < kBinsUnroll; ++u) bins_load<DT, PX>(z + (size_t)(c + u) * hw, i, v[u]);
        group(c, std::integral_constant<int, kBinsUnroll>{});
    }
    for (; c < K; ++c) {
        bins_load<DT, PX>(z + (size_t)c * hw, i, v[0]);
        group(c, std::integral_constant<int, 1>{});
    }
}

template <int DT, int PX>
__global__ __launch_bounds__(kBlock) void bin_loss_grad_kernel(const BinLossGradArgs a) {
    int x, y;
    if (!tile_pixel<PX>(a.tiles_x, a.H, a.W, x, y)) return;
    const size_t b = blockIdx.y, hw = (size_t)a.H * a.W, o = (size_t)y * a.W + x;
    if (a.gup) head_grad<DT, PX>(a.upl, a.Ku, a.upc, a.scale[b * 2], b, hw, o, a.lse + b * 2 * hw, a.bins + b * 2 * hw, a.gup);
    if (a.glat) {
        head_grad<DT, PX>(a.latl, a.Kl, a.latc, a.scale[b * 2 + 1], b, hw, o, a.lse + (b * 2 + 1) * hw, a.bins + (b * 2 + 1) * hw, a.glat);
    }
}

// Pixels per lane of a call (host): the 16-byte access of the logits' type -- 4 float32, 8 16-bit -- where W is a multiple
// of it and every plane given is 16-byte aligned (the planes of every image then are), else 1.
int bin_pixels_per_lane(int dtype, int W, std::initializer_list<const void*> planes) {
    const int px = bins_vec(dtype);
    uintptr_t bits = 0;
    for (const void* p : planes) bits |= reinterpret_cast<uintptr_t>(p);
    return W % px == 0 && bits % 16 == 0 ? px : 1;
}

// Where the logits' type and the pixels per lane become template arguments: f(DT, PX) as integral constants.  Host code.
template <typename F>
hipError_t with_logits(int dtype, int px, F&& f) {
    auto width = [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        return px == 1 ? f(dt, std::integral_constant<int, 1>{}) : f(dt, std::integral_constant<int, bins_vec(DT)>{});
    };
    if (dtype == GCLM_LOGITS_F32) return width(std::integral_constant<int, GCLM_LOGITS_F32>{});
    if (dtype == GCLM_LOGITS_F16) return width(std::integral_constant<int, GCLM_LOGITS_F16>{});
    return width(std::integral_constant<int, GCLM_LOGITS_BF16>{});
}

#pragma clang fp contract(fast)

}  // namespace

size_t bin_loss_workspace(int B, int H, int W) {
    return call_sizes_fit(B, H, W) ? tile_record_bytes(B, H, W, kBinWords, sizeof(float)) : 0;
}

hipError_t launch_bin_loss(int camera_model, const float* cam, const float* grav, int B, int H, int W, const void* up_logits, int Ku,
                           const void* lat_logits, int Kl, int dtype, const float* upc, const float* latc, void* workspace, float* out,
                           float* lse, int16_t* bins, hipStream_t st) {
    const int px = bin_pixels_per_lane(dtype, W, {up_logits, lat_logits, upc, latc, lse, bins});
    const BinLossArgs a{cam, grav, up_logits, lat_logits, upc, latc, static_cast<float*>(workspace), lse, bins,
                        H, W, tile_columns(W, px), tile_columns(W, 1), Ku, Kl};
    return with_camera_model(camera_model, [&](auto m) {
        return with_logits(dtype, px, [&](auto dt, auto p) {
            hipLaunchKernelGGL((bin_loss_kernel<decltype(m)::value, decltype(dt)::value, decltype(p)::value>), dim3(tile_count(H, W, px), B),
                               dim3(kBlock), 0, st, a);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(bin_loss_finish_kernel, dim3(B), dim3(kBlock), 0, st, static_cast<const float*>(workspace),
                               tile_count(H, W, 1), H * W, up_logits != nullptr, upc != nullptr, lat_logits != nullptr, latc != nullptr, out);
            return hipGetLastError();
        });
    });
}

hipError_t launch_bin_loss_grad(int B, int H, int W, const void* up_logits, int Ku, const void* lat_logits, int Kl, int dtype,
                                const float* upc, const float* latc, const float* lse, const int16_t* bins, const float* scale,
                                void* grad_up, void* grad_lat, hipStream_t st) {
    // (a head without its gradient is not read: its planes do not decide the path)
    const int px = bin_pixels_per_lane(dtype, W, {grad_up ? up_logits : nullptr, grad_up ? upc : nullptr, grad_lat ? lat_logits : nullptr,
                                                  grad_lat ? latc : nullptr, lse, bins, grad_up, grad_lat});
    const BinLossGradArgs a{up_logits, lat_logits, upc, latc, lse, scale, bins, grad_up, grad_lat, H, W, tile_columns(W, px), Ku, Kl};
    return with_logits(dtype, px, [&](auto dt, auto p) {
        hipLaunchKernelGGL((bin_loss_grad_kernel<decltype(dt)::value, decltype(p)::value>), dim3(tile_count(H, W, px), B), dim3(kBlock), 0,
                           st, a);
        return hipGetLastError();
    });
}

}  // namespace gclm
