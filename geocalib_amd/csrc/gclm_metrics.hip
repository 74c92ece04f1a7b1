// gclm_metrics.hip -- gclm_field_errors: how well predicted perspective fields agree with a calibration, per image, in one
// pass over the planes (the reference's up_error / latitude_error, siclib/models/utils/metrics.py:95-123, and the decoders'
// metrics built on them, up_decoder.py:111-128, latitude_decoder.py:116-133, with the target fields of
// get_perspective_field evaluated per pixel in registers instead of rendered to memory and read back).
//
// Per pixel, with t_up (normalised) and t_lat the target of gclm_render.h's persp_up / persp_lat at the camera and gravity:
//   up:  e = deg(angle(p, t_up)) * mask,  mask = (p_x + p_y != 0) in float32 (up_decoder.py:115, as written)
//        angle = acos(clamp(F.cosine_similarity(p, t, dim=1), -1, 1)): with P = p / max(|p|, 1e-8), T = t / max(|t|, 1e-8),
//        the cosine is P . T.  Where both norms reach 1e-8 the angle is atan2(|p x t|, p . t), which resolves small angles
//        (float32 acos cannot: acos(1 - 2^-24) = 0.02 deg is its smallest non-zero value); otherwise |P| |T| < 1 and the
//        angle is atan2(sqrt((1 - |P|^2 |T|^2) + (P x T)^2), P . T), the same acos written without the cancellation.
//   lat: e = |lat - t_lat| * 180 / pi
// A masked pixel has error 0 (a hit at every threshold); a NaN prediction gives a NaN error (NaN * 0 stays NaN), which
// makes the image's sums NaN and counts at no threshold.
//
// Per image: mean = sum e / (H W), weighted = sum(e conf) / sum conf, recall@t = #(e < t) / (H W).
//
// Layout: the tile walk of gclm_render.h ("The tile walk": tile geometry, pixels per lane, wave sum, one record per tile, a
// finish kernel of strided float64 chains), grid = (tiles of one image, B).  What is this file's own: the counts are ballots
// (wave-uniform integers) that lane 0 leaves in LDS next to the wave's float sums, and the record of a tile is
//   words [0, 6): float sum e_up, sum e_up c_up, sum c_up, sum e_lat, sum e_lat c_lat, sum c_lat;  then n_thresholds
//   uint32 counts of up, then of latitude,
// so field_error_finish_kernel (grid = B, eight chains) walks words of two types and keeps chain_sum's loop written out.
// The u, r2 loop of a lane's pixels is written out as well (as field_loss.hip's lane_row has it: through a shared function
// field_error_kernel's instruction streams change).  64-bit offsets.  No scratch.
// Measured (both confidences, four against two pixels per lane in one process): -5 % (pinhole) /
// -1 .. 0 % (simple_divisional) kernel time at B = 1024, -13 % / -9 % at B = 16: four kept.
#include "gclm_render.h"

namespace gclm {
namespace {

constexpr int kMaxThr = GCLM_MAX_RECALL_THRESHOLDS;
constexpr int kSumWords = 6;                 // float sums per record; 2 n_thresholds counts follow
constexpr int kChains = 8;                   // summation chains per image of the second launch

struct FieldErrArgs {
    const float *cam, *grav, *up, *lat, *upc, *latc;
    float *up_err, *lat_err;
    uint32_t* rec;
    int H, W, tiles_x, nth;
    float thr[kMaxThr];
};

template <int MODEL, int PX>
__global__ __launch_bounds__(kBlock) void field_error_kernel(const FieldErrArgs a) {
    __shared__ float s_sum[kTileRows][kSumWords];
    __shared__ uint32_t s_cnt[kTileRows][2 * kMaxThr];
    int x, y;
    const bool in = tile_pixel<PX>(a.tiles_x, a.H, a.W, x, y);
    const int b = blockIdx.y, wave = threadIdx.x >> 6;
    const float nan = __builtin_nanf("");
    float e_up[PX], e_lat[PX];
    float sum[kSumWords] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < PX; ++j) e_up[j] = e_lat[j] = nan;      // a lane outside the image counts at no threshold
    if (in) {
        const PerspRow r = persp_row(a.cam + (size_t)b * 8, a.grav + (size_t)b * 3, y);
        const size_t hw = (size_t)a.H * a.W, o = (size_t)b * hw + (size_t)y * a.W + x;
        float u[PX], r2[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            u[j] = ((float)(x + j) - r.cx) * r.ifx;
            r2[j] = u[j] * u[j] + r.v2;
        }
        if (a.up) {
            float px[PX], py[PX];
            load_px<PX>(a.up + o + (size_t)b * hw, px);          // (B, 2, H, W): image b starts at 2 b H W
            load_px<PX>(a.up + o + (size_t)b * hw + hw, py);
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                e_up[j] = up_error_deg(px[j], py[j], persp_up<MODEL>(r, u[j], r2[j], true));
                sum[0] += e_up[j];
            }
            if (a.upc) {
                float c[PX];
                load_px<PX>(a.upc + o, c);
#pragma unroll
                for (int j = 0; j < PX; ++j) sum[1] += e_up[j] * c[j], sum[2] += c[j];
            }
            if (a.up_err) store_px<PX>(e_up, a.up_err + o);
        }
        if (a.lat) {
            float l[PX];
            load_px<PX>(a.lat + o, l);
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                e_lat[j] = fabsf(l[j] - persp_lat<MODEL>(r, u[j], r2[j])) * kDegrees;
                sum[3] += e_lat[j];
            }
            if (a.latc) {
                float c[PX];
                load_px<PX>(a.latc + o, c);
#pragma unroll
                for (int j = 0; j < PX; ++j) sum[4] += e_lat[j] * c[j], sum[5] += c[j];
            }
            if (a.lat_err) store_px<PX>(e_lat, a.lat_err + o);
        }
    }
    // every lane of the block from here on: wave sums, wave-uniform counts, one record per wave in LDS
#pragma unroll
    for (int k = 0; k < kSumWords; ++k) sum[k] = wave_sum(sum[k]);
    uint32_t cnt[2 * kMaxThr];
#pragma unroll
    for (int k = 0; k < kMaxThr; ++k) {
        uint32_t nu = 0, nl = 0;
        if (k < a.nth) {
            const float t = a.thr[k];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                nu += (uint32_t)__popcll(__ballot(e_up[j] < t));
                nl += (uint32_t)__popcll(__ballot(e_lat[j] < t));
            }
        }
        cnt[k] = nu, cnt[kMaxThr + k] = nl;
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kSumWords; ++k) s_sum[wave][k] = sum[k];
#pragma unroll
        for (int k = 0; k < 2 * kMaxThr; ++k) s_cnt[wave][k] = cnt[k];
    }
    __syncthreads();
    const int k = threadIdx.x, words = kSumWords + 2 * a.nth;
    if (k < words) {
        uint32_t w;
        if (k < kSumWords) {
            w = __float_as_uint(column_sum(s_sum, k));
        } else {
            const int c = k - kSumWords, col = c < a.nth ? c : kMaxThr + (c - a.nth);
            w = 0;
            for (int i = 0; i < kTileRows; ++i) w += s_cnt[i][col];
        }
        a.rec[((size_t)b * gridDim.x + blockIdx.x) * words + k] = w;
    }
}

// One block per image: word k of the image's records is summed by kChains chains (record t goes to chain t % kChains), the
// chains are added in order, all in float64 (the counts are exact in it).  stats (B, 2 (2 + nth)), file header.
__global__ __launch_bounds__(kBlock) void field_error_finish_kernel(const uint32_t* __restrict__ rec, int tiles, int nth, int hw,
                                                                    int has_up, int has_upc, int has_lat, int has_latc,
                                                                    float* __restrict__ stats) {
    __shared__ double part[kChains][32];
    const int b = blockIdx.x, k = threadIdx.x & 31, chain = threadIdx.x >> 5, words = kSumWords + 2 * nth;
    double acc = 0.0;
    if (k < words) {
        const uint32_t* p = rec + (size_t)b * tiles * words + k;
        for (int t = chain; t < tiles; t += kChains) {       // chain_sum's walk, over words of two types
            const uint32_t w = p[(size_t)t * words];
            acc += k < kSumWords ? (double)__uint_as_float(w) : (double)w;
        }
    }
    part[chain][k] = acc;
    __syncthreads();
    if (threadIdx.x < 32) {
        const double s = column_sum(part, k);
        part[0][k] = s;
    }
    __syncthreads();
    const int per = 2 + nth, i = threadIdx.x;
    if (i < 2 * per) {
        const int field = i / per, m = i - field * per;
        const bool has = field ? has_lat != 0 : has_up != 0, hasc = field ? has_latc != 0 : has_upc != 0;
        double v;
        if (m == 0) v = part[0][3 * field] / (double)hw;
        else if (m == 1) v = hasc ? part[0][3 * field + 1] / part[0][3 * field + 2] : (double)__builtin_nanf("");
        else v = part[0][kSumWords + field * nth + (m - 2)] / (double)hw;
        stats[(size_t)b * 2 * per + i] = has ? (float)v : __builtin_nanf("");
    }
}

// The most pixels per lane: a build with -DGCLM_METRICS_MAX_PX=2 is the measured alternative (scripts/field_metrics_bench.py
// --variant-lib times such a build against this one).
#ifndef GCLM_METRICS_MAX_PX
#define GCLM_METRICS_MAX_PX 4
#endif

}  // namespace

size_t field_errors_workspace(int B, int H, int W, int n_thresholds) {
    if (!call_sizes_fit(B, H, W) || n_thresholds < 0 || n_thresholds > kMaxThr) return 0;
    return tile_record_bytes(B, H, W, kSumWords + 2 * n_thresholds, sizeof(uint32_t));
}

hipError_t launch_field_errors(int camera_model, const float* cam, const float* grav, int B, int H, int W, const float* up,
                               const float* lat, const float* upc, const float* latc, int n_thresholds, const float* thresholds,
                               void* workspace, float* stats, float* up_err, float* lat_err, hipStream_t st) {
    const int px = pixels_per_lane(W, {up, lat, upc, latc, up_err, lat_err}, GCLM_METRICS_MAX_PX);
    FieldErrArgs a{cam, grav, up, lat, upc, latc, up_err, lat_err, static_cast<uint32_t*>(workspace), H, W, tile_columns(W, px),
                   n_thresholds, {}};
    for (int k = 0; k < n_thresholds; ++k) a.thr[k] = thresholds[k];
    const int tiles = tile_count(H, W, px);
    return with_camera_model(camera_model, [&](auto m) {
        constexpr int M = decltype(m)::value;
        const auto kernel = with_pixels_per_lane<GCLM_METRICS_MAX_PX>(px, [](auto p) { return field_error_kernel<M, decltype(p)::value>; });
        hipLaunchKernelGGL(kernel, dim3(tiles, B), dim3(kBlock), 0, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(field_error_finish_kernel, dim3(B), dim3(kBlock), 0, st, static_cast<const uint32_t*>(workspace), tiles,
                           n_thresholds, H * W, up != nullptr, upc != nullptr, lat != nullptr, latc != nullptr, stats);
        return hipGetLastError();
    });
}

}  // namespace gclm
