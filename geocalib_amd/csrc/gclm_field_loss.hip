// gclm_field_loss.hip -- gclm_field_loss / gclm_field_loss_grad: the losses the up and latitude heads are trained with, per
// image, and their gradients with respect to the predicted fields (the reference's UpDecoder.calculate_losses /
// LatitudeDecoder.calculate_losses, siclib/models/decoders/up_decoder.py:51-79, latitude_decoder.py:53-79), with the target
// fields of get_perspective_field evaluated per pixel in registers (gclm_render.h: persp_up normalised, persp_lat) instead
// of rendered to memory, read back by a dozen eager kernels and replayed backwards by autograd.
//
// Per pixel of one field, r = p - t per component (up: 2, latitude: 1), with s = sum_c r_c^2:
//   l1      l = sum_c |r_c|                                   dl/dp_c = sign(r_c), 0 at 0 (a NaN stays NaN)
//   l2      l = s                                             dl/dp_c = 2 r_c
//   dot     l = 1 - sum_c r_c t_c  (up only; on the residual, as the reference writes it)   dl/dp_c = -t_c
//   cauchy  l = c^2 / 2 log1p(s / c^2), c = 0.007             dl/dp_c = r_c / (1 + s / c^2)
//   huber   l = sum_c h(r_c), delta = pi / 180: h = r^2 / 2 for |r| < delta, else delta (|r| - delta / 2)
//                                                             dl/dp_c = clamp(r_c, -delta, delta) (a NaN stays NaN)
// Per image: loss = sum l / (H W), or sum(l conf) / sum conf where that confidence is given (the reference's
// loss * (conf / sum conf * H W) followed by .mean(), the confidence detached).  The gradient of a pixel is
// scale[b, field] * dl/dp_c, times conf where given; the caller forms scale = grad_output * weight / denominator from the
// forward's d_out.  Nothing but the inputs lives between the two calls: the gradient call evaluates the target again.
//
// Forward: the tile walk of gclm_render.h ("The tile walk"), with a record of four float sums per tile: sum l_up (x c_up),
// sum c_up, sum l_lat (x c_lat), sum c_lat; field_loss_finish_kernel (grid = B) sums them in eight chains.
// Gradient: the same walk with no reduction, no LDS, no barrier; plain stores (the planes are read next, by autograd).
// The loss type is a kernel argument taken by a branch every lane of the grid takes alike, not a template parameter:
// camera model x PX instantiations per kernel.  Pixels per lane by gclm_render.h's pixels_per_lane.  64-bit offsets.  No scratch.
// pixel_loss, pixel_grad and lane_row are gclm_field_loss.h's, shared with gclm_field_param_grad.hip.
#include "gclm_field_loss.h"

namespace gclm {
namespace {

constexpr int kLossWords = 4;                // float sums per record
constexpr int kLossChains = 8;               // summation chains per image of the second launch

struct FieldLossArgs {
    const float *cam, *grav, *up, *lat, *upc, *latc;
    float* rec;
    int H, W, tiles_x, up_loss, lat_loss;
};

struct FieldLossGradArgs {
    const float *cam, *grav, *up, *lat, *upc, *latc, *scale;
    float *grad_up, *grad_lat;
    int H, W, tiles_x, up_loss, lat_loss;
};

// The gradient planes' stores: plain, since autograd reads the planes next.  A build with -DGCLM_FIELD_LOSS_NT_STORES=1 is the
// measured alternative (scripts/field_loss_bench.py --variant-lib times such a build against this one).
#ifndef GCLM_FIELD_LOSS_NT_STORES
#define GCLM_FIELD_LOSS_NT_STORES 0
#endif

constexpr bool kGradNT = GCLM_FIELD_LOSS_NT_STORES != 0;

template <int MODEL, int PX>
__global__ __launch_bounds__(kBlock) void field_loss_kernel(const FieldLossArgs a) {
    __shared__ float s_sum[kTileRows][kLossWords];
    int x, y;
    const bool in = tile_pixel<PX>(a.tiles_x, a.H, a.W, x, y);
    const int b = blockIdx.y, wave = threadIdx.x >> 6;
    float sum[kLossWords] = {0.f, 0.f, 0.f, 0.f};
    if (in) {
        float u[PX], r2[PX];
        const PerspRow r = lane_row<PX>(a.cam, a.grav, b, x, y, u, r2);
        const size_t hw = (size_t)a.H * a.W, o = (size_t)b * hw + (size_t)y * a.W + x;
        if (a.up) {
            float px[PX], py[PX], l[PX];
            load_px<PX>(a.up + o + (size_t)b * hw, px);          // (B, 2, H, W): image b starts at 2 b H W
            load_px<PX>(a.up + o + (size_t)b * hw + hw, py);
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const f32x2 t = persp_up<MODEL>(r, u[j], r2[j], true);
                const float tt[2] = {t.x, t.y}, rr[2] = {px[j] - t.x, py[j] - t.y};
                l[j] = pixel_loss<2>(a.up_loss, rr, tt);
            }
            if (a.upc) {
                float c[PX];
                load_px<PX>(a.upc + o, c);
#pragma unroll
                for (int j = 0; j < PX; ++j) sum[0] += l[j] * c[j], sum[1] += c[j];
            } else {
#pragma unroll
                for (int j = 0; j < PX; ++j) sum[0] += l[j];
            }
        }
        if (a.lat) {
            float p[PX], l[PX];
            load_px<PX>(a.lat + o, p);
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const float tt[1] = {persp_lat<MODEL>(r, u[j], r2[j])}, rr[1] = {p[j] - tt[0]};
                l[j] = pixel_loss<1>(a.lat_loss, rr, tt);
            }
            if (a.latc) {
                float c[PX];
                load_px<PX>(a.latc + o, c);
#pragma unroll
                for (int j = 0; j < PX; ++j) sum[2] += l[j] * c[j], sum[3] += c[j];
            } else {
#pragma unroll
                for (int j = 0; j < PX; ++j) sum[2] += l[j];
            }
        }
    }
    // every lane of the block from here on: wave sums, one record per wave in LDS, one per tile in the workspace
#pragma unroll
    for (int k = 0; k < kLossWords; ++k) sum[k] = wave_sum(sum[k]);
    tile_record(s_sum, wave, sum, [&](int k, float s) { a.rec[((size_t)b * gridDim.x + blockIdx.x) * kLossWords + k] = s; });
}

// One block per image: word k of the image's records is summed by kLossChains chains (record t goes to chain
// t % kLossChains), the chains are added in order, all in float64.  out (B, 4) = [up loss, latitude loss, up denominator,
// latitude denominator]: the denominator is H W, or sum conf where that confidence is given; NaN for an absent field.
__global__ __launch_bounds__(kBlock) void field_loss_finish_kernel(const float* __restrict__ rec, int tiles, int hw, int has_up,
                                                                   int has_upc, int has_lat, int has_latc, float* __restrict__ out) {
    __shared__ double part[kLossChains][kLossWords];
    const int b = blockIdx.x, k = threadIdx.x & 31, chain = threadIdx.x >> 5;
    if (k < kLossWords) {
        part[chain][k] = chain_sum<kLossChains>(rec + (size_t)b * tiles * kLossWords + k, kLossWords, tiles, chain);
    }
    __syncthreads();
    const int field = threadIdx.x;
    if (field < 2) {
        double num = column_sum(part, 2 * field), den = column_sum(part, 2 * field + 1);
        const bool has = field ? has_lat != 0 : has_up != 0, hasc = field ? has_latc != 0 : has_upc != 0;
        if (!hasc) den = (double)hw;
        out[(size_t)b * 4 + field] = has ? (float)(num / den) : __builtin_nanf("");
        out[(size_t)b * 4 + 2 + field] = has ? (float)den : __builtin_nanf("");
    }
}

template <int MODEL, int PX>
__global__ __launch_bounds__(kBlock) void field_loss_grad_kernel(const FieldLossGradArgs a) {
    int x, y;
    if (!tile_pixel<PX>(a.tiles_x, a.H, a.W, x, y)) return;
    const int b = blockIdx.y;
    float u[PX], r2[PX];
    const PerspRow r = lane_row<PX>(a.cam, a.grav, b, x, y, u, r2);
    const size_t hw = (size_t)a.H * a.W, o = (size_t)b * hw + (size_t)y * a.W + x;
    if (a.up) {
        const float scale = a.scale[(size_t)b * 2];
        float px[PX], py[PX], gx[PX], gy[PX];
        load_px<PX>(a.up + o + (size_t)b * hw, px);
        load_px<PX>(a.up + o + (size_t)b * hw + hw, py);
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const f32x2 t = persp_up<MODEL>(r, u[j], r2[j], true);
            const float tt[2] = {t.x, t.y}, rr[2] = {px[j] - t.x, py[j] - t.y};
            float g[2];
            pixel_grad<2>(a.up_loss, rr, tt, g);
            gx[j] = scale * g[0], gy[j] = scale * g[1];
        }
        if (a.upc) {
            float c[PX];
            load_px<PX>(a.upc + o, c);
#pragma unroll
            for (int j = 0; j < PX; ++j) gx[j] *= c[j], gy[j] *= c[j];
        }
        store_px<PX, kGradNT>(gx, a.grad_up + o + (size_t)b * hw);
        store_px<PX, kGradNT>(gy, a.grad_up + o + (size_t)b * hw + hw);
    }
    if (a.lat) {
        const float scale = a.scale[(size_t)b * 2 + 1];
        float p[PX], gl[PX];
        load_px<PX>(a.lat + o, p);
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const float tt[1] = {persp_lat<MODEL>(r, u[j], r2[j])}, rr[1] = {p[j] - tt[0]};
            float g[1];
            pixel_grad<1>(a.lat_loss, rr, tt, g);
            gl[j] = scale * g[0];
        }
        if (a.latc) {
            float c[PX];
            load_px<PX>(a.latc + o, c);
#pragma unroll
            for (int j = 0; j < PX; ++j) gl[j] *= c[j];
        }
        store_px<PX, kGradNT>(gl, a.grad_lat + o);
    }
}

}  // namespace

size_t field_loss_workspace(int B, int H, int W) {
    return call_sizes_fit(B, H, W) ? tile_record_bytes(B, H, W, kLossWords, sizeof(float)) : 0;
}

hipError_t launch_field_loss(int camera_model, const float* cam, const float* grav, int B, int H, int W, const float* up,
                             const float* lat, const float* upc, const float* latc, int up_loss, int lat_loss, void* workspace,
                             float* out, hipStream_t st) {
    const int px = pixels_per_lane(W, {up, lat, upc, latc});
    const FieldLossArgs a{cam, grav, up, lat, upc, latc, static_cast<float*>(workspace), H, W, tile_columns(W, px), up_loss, lat_loss};
    const int tiles = tile_count(H, W, px);
    return with_camera_model(camera_model, [&](auto m) {
        constexpr int M = decltype(m)::value;
        const auto kernel = with_pixels_per_lane(px, [](auto p) { return field_loss_kernel<M, decltype(p)::value>; });
        hipLaunchKernelGGL(kernel, dim3(tiles, B), dim3(kBlock), 0, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(field_loss_finish_kernel, dim3(B), dim3(kBlock), 0, st, static_cast<const float*>(workspace), tiles, H * W,
                           up != nullptr, upc != nullptr, lat != nullptr, latc != nullptr, out);
        return hipGetLastError();
    });
}

hipError_t launch_field_loss_grad(int camera_model, const float* cam, const float* grav, int B, int H, int W, const float* up,
                                  const float* lat, const float* upc, const float* latc, int up_loss, int lat_loss, const float* scale,
                                  float* grad_up, float* grad_lat, hipStream_t st) {
    const int px = pixels_per_lane(W, {up, lat, upc, latc, grad_up, grad_lat});
    const FieldLossGradArgs a{cam, grav, up, lat, upc, latc, scale, grad_up, grad_lat, H, W, tile_columns(W, px), up_loss, lat_loss};
    return with_camera_model(camera_model, [&](auto m) {
        constexpr int M = decltype(m)::value;
        const auto kernel = with_pixels_per_lane(px, [](auto p) { return field_loss_grad_kernel<M, decltype(p)::value>; });
        hipLaunchKernelGGL(kernel, dim3(tile_count(H, W, px), B), dim3(kBlock), 0, st, a);
        return hipGetLastError();
    });
}

}  // namespace gclm
