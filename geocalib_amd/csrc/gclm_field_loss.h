// gclm_field_loss.h -- what the kernels of the decoders' losses share: the per-pixel loss and its derivative with respect to
// the prediction (the table in gclm_field_loss.hip's header and include/gclm.h: gclm_field_loss), and the row terms of a
// lane's pixels.  Included by gclm_field_loss.hip (the losses and their gradients to the predicted fields) and by
// gclm_field_param_grad.hip (their gradients to the camera and the gravity).
#pragma once
#include "gclm_render.h"

namespace gclm {

constexpr float kCauchyC2 = 0.007f * 0.007f;
constexpr float kHuberDelta = 0.017453292519943295f;          // deg2rad(1)

__device__ __forceinline__ float huber(float r) {
    const float a = fabsf(r);
    return a < kHuberDelta ? 0.5f * r * r : kHuberDelta * (a - 0.5f * kHuberDelta);      // (a NaN takes the second arm: NaN)
}

// l of one pixel: r and t hold its C components
template <int C>
__device__ __forceinline__ float pixel_loss(int type, const float (&r)[C], const float (&t)[C]) {
    float s = 0.f;
    switch (type) {
        case GCLM_FIELD_LOSS_L1:
#pragma unroll
            for (int c = 0; c < C; ++c) s += fabsf(r[c]);
            return s;
        case GCLM_FIELD_LOSS_DOT:
#pragma unroll
            for (int c = 0; c < C; ++c) s += r[c] * t[c];
            return 1.f - s;
        case GCLM_FIELD_LOSS_HUBER:
#pragma unroll
            for (int c = 0; c < C; ++c) s += huber(r[c]);
            return s;
        default:
#pragma unroll
            for (int c = 0; c < C; ++c) s += r[c] * r[c];
            return type == GCLM_FIELD_LOSS_L2 ? s : (0.5f * kCauchyC2) * log1pf(s / kCauchyC2);
    }
}

// dl/dp_c of one pixel, into g
template <int C>
__device__ __forceinline__ void pixel_grad(int type, const float (&r)[C], const float (&t)[C], float (&g)[C]) {
    switch (type) {
        case GCLM_FIELD_LOSS_L1:
#pragma unroll
            for (int c = 0; c < C; ++c) g[c] = r[c] > 0.f ? 1.f : (r[c] < 0.f ? -1.f : (r[c] == 0.f ? 0.f : r[c]));
            return;
        case GCLM_FIELD_LOSS_L2:
#pragma unroll
            for (int c = 0; c < C; ++c) g[c] = 2.f * r[c];
            return;
        case GCLM_FIELD_LOSS_DOT:
#pragma unroll
            for (int c = 0; c < C; ++c) g[c] = -t[c];
            return;
        case GCLM_FIELD_LOSS_HUBER:
#pragma unroll
            for (int c = 0; c < C; ++c) g[c] = r[c] < -kHuberDelta ? -kHuberDelta : (r[c] > kHuberDelta ? kHuberDelta : r[c]);
            return;
        default: {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) s += r[c] * r[c];
            const float w = 1.f / (1.f + s / kCauchyC2);
#pragma unroll
            for (int c = 0; c < C; ++c) g[c] = r[c] * w;
        }
    }
}

// The row's terms of this lane's pixels (x, y), and u, r2 of each of them.
template <int PX>
__device__ __forceinline__ PerspRow lane_row(const float* cam, const float* grav, int b, int x, int y, float (&u)[PX], float (&r2)[PX]) {
    const PerspRow r = persp_row(cam + (size_t)b * 8, grav + (size_t)b * 3, y);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        u[j] = ((float)(x + j) - r.cx) * r.ifx;
        r2[j] = u[j] * u[j] + r.v2;
    }
    return r;
}

}  // namespace gclm
