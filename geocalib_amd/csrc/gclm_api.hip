// gclm_api.hip -- the handle of libgeocalib_hip.so's C ABI (include/gclm.h), the plan and the launch sequence of a solve, with
// the entry points that take a handle (those that take none: gclm_entry.hip).
//
// A solve is 2*num_steps+4 asynchronous launches on the caller's stream and no host round trip (nor memset):
//   init | { sweep(theta_i) ; update_i } x num_steps | prep_final ; sweep(theta_final, rpf) ; finalize
// and num_steps+2 for a single image (one launch per LM step, make_plan; the first launch builds theta_0 itself):
//   fused(step) x num_steps | fused(final) | finalize
// (the reference syncs twice per step: H,G -> CPU Cholesky -> device, and torch.allclose).
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "gclm_args.h"
#include "gclm_internal.h"

using namespace gclm;

#ifndef GCLM_FUSED_MAX_WORKGROUPS
#define GCLM_FUSED_MAX_WORKGROUPS 768      // B * workgroups-per-image up to which an LM step is ONE launch (see choose_walk):
                                           // measured with round 4's prologue (profiles/archive/r04_fused_threshold.log, 20 fixed steps) --
                                           // 640x480 (150 workgroups per image): B = 2 -19 %, 4 -15 %, 6 +-0, 8 +6 %, 12 +15 %;
                                           // 320x240 (38 per image): B = 2 ... 12 -20 ... -27 %
#endif
#ifndef GCLM_ROW_PAIRS_DEFAULT
#define GCLM_ROW_PAIRS_DEFAULT -1   // a handle's initial gclm_set_row_pairs mode (1: test builds that run the whole suite on row pairs)
#endif
#ifndef GCLM_CONF_PACK_MIN_PIXELS
#define GCLM_CONF_PACK_MIN_PIXELS (256ll << 20)  // B * H * W from which a pinhole solve packs its confidence planes on its own (wants_conf_pack)
#endif
#ifndef GCLM_ISO_FINAL
#define GCLM_ISO_FINAL 1      // A/B switch: 0 = the final sweep always takes the general focal column
#endif

namespace {

// The field planes of one call (device pointers; every one but `lat` may be null)
struct Fields {
    const float *up = nullptr, *lat = nullptr, *upc = nullptr, *latc = nullptr;
    bool five() const { return up && upc && latc; }       // a complete field set: (B,2,H,W) + four (B,H,W) planes
    bool aligned16() const { return is_aligned(up, 16) && is_aligned(lat, 16) && is_aligned(upc, 16) && is_aligned(latc, 16); }
};

// Everything decided ONCE per call about its sweeps (make_plan): how they walk the image, whether an LM step is one launch,
// and which plane of sin(latitude) they read.  A solve keeps it as a local; the split shared-intrinsics session keeps it
// on the handle between its calls (gclm_handle::sh).
struct Plan {
    Fields f;
    Geometry geo{};                 // the one-row walk, or row pairs (geo.mirror)
    bool one_launch = false;        // an LM step is ONE launch (gclm_pass.hip: fused_step_kernel); never with row pairs
    const float* given = nullptr;   // the caller's plane of sin(latitude) every sweep reads in place of `lat`, or null
    float* slat = nullptr;          // else the library's scratch plane (gclm_handle::slat), or null: sweeps compute sin(latitude)
    bool slat_filled = false;       // ... which the first sweep fills and the later ones read (next_sweep)
    uint32_t* cpack = nullptr;      // the library's plane of packed confidences (gclm_handle::cpack), or null: sweeps read the caller's two
    bool cpack_filled = false;      // ... filled by the first sweep, read by the later ones, like `slat`; never both planes in one solve

    void choose_walk(const gclm_handle* h, int B, int H, int W, bool aligned16, bool five);
    SweepArgs next_sweep(const gclm_handle* h, const PBlock* pb, bool loop_params, int stop_step);
};

}  // namespace

struct gclm_handle {
    gclm_config cfg;
    int device = 0;
    std::string err;
    // device scratch (owned)
    void* ws = nullptr;
    size_t ws_bytes = 0;
    // carved views
    SolveCtx ctx{};
    float* group_partials = nullptr;
    float* prior_cost = nullptr;    // (B,2) the soft priors' costs of a gclm_calibrate_soft call that hands no d_prior_cost_out
    // split shared-intrinsics session
    struct {
        bool active = false;
        Plan plan;                  // of gclm_shared_begin: every gclm_shared_reduce and gclm_shared_finish takes its next sweep from it
        float *cam_io = nullptr, *grav_io = nullptr;
    } sh;
    // The two scratch planes -- sin(latitude) for the distortion models, the packed confidences for pinhole -- are allocations of
    // their own, of exactly the size asked for (no headroom), and the only parts of the workspace a solve can do without: see
    // ensure_plane.
    struct ScratchPlane {
        void* buf = nullptr;        // owned: `bytes` bytes, or null
        size_t bytes = 0;
        size_t refused = 0;         // smallest plane size (bytes) whose allocation failed or was refused by the limit since the
                                    // last change of the limit / mode: such a size is not tried again on every solve ...
        int refused_asks = 0;       // ... but after kRefusalAsks solves that wanted it (memory others held may be free again)
    } slat, cpack;
    size_t slat_limit = 0;          // gclm_set_slat_plane_limit (either plane): 0 = built-in rule (half of the free device memory), else bytes
    int slat_plane = -1;            // gclm_set_slat_plane: -1 = built-in choice, 0 = never, 1 = wherever the sweep has it
    int conf_pack = -1;             // gclm_set_conf_pack: -1 = built-in choice, 0 = never, 1 = wherever the sweep has it
    int cpack_images = 0;           // images of the last solve if it packed its confidences, else 0 (gclm_conf_pack_fallbacks)
    int row_pairs = GCLM_ROW_PAIRS_DEFAULT;   // gclm_set_row_pairs: -1 = built-in choice, 0 = never, 1 = wherever the sweep has the row-pair walk
    int sweep_iters = 0;            // gclm_set_sweep_iters: 0 = built-in choice
    int fused_mode = -1;            // gclm_set_fused_steps: -1 = built-in choice, 0 = never, 1 = whenever it is valid
    gclm_comm* stop_comm = nullptr; // gclm_set_stop_comm: the batch-global early stop spans the ranks of this communicator
    int paced_depth = 0;            // gclm_set_paced_launches: 0 = off, d = launch k waits for launch k-d's report
    unsigned* progress_host = nullptr;   // ... the host-mapped word the launches report to (owned), its device alias
    unsigned* progress_dev = nullptr;
    unsigned epoch = 0;             // ... and the tag of the current solve in it
    int paced_cooldown = 0;         // solves left to run UNPACED after a wait timed out (the queue was not ours)
    // optional timing of the sweep launches
    bool timing = false;
    std::vector<hipEvent_t> ev;
    int ev_used = 0;
};

namespace {

thread_local std::string g_create_error;

int fail(gclm_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

#define GCLM_HIP(h, expr)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return fail(h, -10, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// A caller built against another include/gclm.h must be told so, not trusted with a struct of another layout.
const char* abi_mismatch(const gclm_config* c, char (&buf)[256]) {
    if (c->struct_size == (int32_t)sizeof(gclm_config) && c->abi_version == GCLM_VERSION) return nullptr;
    snprintf(buf, sizeof(buf), "gclm_config ABI mismatch: caller passes struct_size %d / abi_version %d, this library is "
             "sizeof(gclm_config) %d / GCLM_VERSION %d (rebuild the caller against this include/gclm.h and fill the "
             "struct with gclm_default_config)", (int)c->struct_size, (int)c->abi_version, (int)sizeof(gclm_config), GCLM_VERSION);
    return buf;
}

const char* validate(const gclm_config& c) {
    if (c.camera_model < GCLM_PINHOLE || c.camera_model > GCLM_SIMPLE_DIVISIONAL)
        return "camera_model: unknown (0 pinhole, 1 simple_radial, 2 radial, 3 simple_divisional)";
    if (c.num_steps < 0 || c.num_steps > GCLM_MAX_STEPS) return "num_steps out of range [0, GCLM_MAX_STEPS]";
    if (!(c.up_loss_fn_scale > 0.f) || !(c.lat_loss_fn_scale > 0.f)) return "loss scales must be > 0";
    if (c.group_size < 0) return "group_size must be >= 0";
    if (c.shared_intrinsics && !(c.estimate_gravity && c.estimate_focal))
        return "shared_intrinsics requires gravity and focal to be estimated (lm_optimizer.py:350-383)";
    if (c.shared_intrinsics && c.camera_model != GCLM_PINHOLE && !c.estimate_dist)
        return "shared_intrinsics with a distortion prior is not supported";
    const int n = 2 * (c.estimate_gravity != 0) + (c.estimate_focal != 0) + num_dist_params(c.camera_model);
    if (n == 0) return "No parameters to optimize";
    return nullptr;
}

// Every entry point runs on the handle's device and leaves the CALLER's current device as it found it (a
// single-process multi-GPU program would otherwise see its default device flip under PyTorch, also at garbage-
// collection time through gclm_destroy).
struct DeviceGuard {
    int prev = -1;
    hipError_t status = hipSuccess;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) status = hipSetDevice(device); else prev = -1;    // prev = -1: nothing to restore
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Carve the core workspace for B images / nchunks partial records per image / G groups.  Growing it frees and re-allocates
// (hipFree synchronises the device ONCE, on the first call of a larger shape than any before; every later call finds the
// workspace in place -- include/gclm.h says so).  A failure here is the only allocation failure a solve reports (-10).
int ensure_workspace(gclm_handle* h, int B, int nchunks, int G) {
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t o_state0 = take(sizeof(State) * B), o_state1 = take(sizeof(State) * B);
    const size_t o_pb0 = take(sizeof(PBlock) * B), o_pb1 = take(sizeof(PBlock) * B), o_pbf = take(sizeof(PBlock) * B);
    const size_t o_part = take(sizeof(float) * kNAccMax * (size_t)B * nchunks);
    const size_t o_part2 = take(sizeof(float) * kNAccMax * (size_t)B * nchunks);     // double buffer of the fused path
    const size_t o_fsys = take(sizeof(float) * kNAccMax * (size_t)B);
    const size_t o_gp = take(sizeof(float) * GCLM_SHARED_PARTIAL_STRIDE * (size_t)(G > 0 ? G : 1));
    const size_t o_ctrl = take(sizeof(Ctrl));
    const size_t o_cpf = take(sizeof(unsigned) * B);
    const size_t o_pc = take(sizeof(float) * 2 * B);
    if (off > h->ws_bytes) {
        if (h->ws) GCLM_HIP(h, hipFree(h->ws));
        h->ws = nullptr;
        h->ws_bytes = 0;
        const size_t want = off + off / 4;      // headroom: no reallocation for slightly larger calls (small records only:
                                                // 3 MB at 1024 images of 640x480; the scratch plane is NOT in here)
        GCLM_HIP(h, hipMalloc(&h->ws, want));
        h->ws_bytes = want;
    }
    char* base = static_cast<char*>(h->ws);
    SolveCtx& c = h->ctx;
    c.state[0] = reinterpret_cast<State*>(base + o_state0);
    c.state[1] = reinterpret_cast<State*>(base + o_state1);
    c.pb[0] = reinterpret_cast<PBlock*>(base + o_pb0);
    c.pb[1] = reinterpret_cast<PBlock*>(base + o_pb1);
    c.pb_final = reinterpret_cast<PBlock*>(base + o_pbf);
    c.partials = reinterpret_cast<float*>(base + o_part);
    c.partials2 = reinterpret_cast<float*>(base + o_part2);
    c.frame_sys = reinterpret_cast<float*>(base + o_fsys);
    c.ctrl = reinterpret_cast<Ctrl*>(base + o_ctrl);
    c.cpack_flags = reinterpret_cast<unsigned*>(base + o_cpf);
    h->group_partials = reinterpret_cast<float*>(base + o_gp);
    h->prior_cost = reinterpret_cast<float*>(base + o_pc);
    return 0;
}

// A scratch plane of `bytes` bytes for this solve (0: none wanted): returns the plane, or null when the solve runs without it
// -- never an error.  Either plane only saves work (gclm_pass.hip: row_math, SLAT / CPACK): the sweeps that do without it are
// the library's own earlier ones, so whenever the plane cannot be had -- hipMalloc fails, or the plane is larger than the limit
// (gclm_set_slat_plane_limit; built-in: half of the device memory that is free once the old plane is released) -- the solve
// goes on without it.  Exact size, no headroom: a plane is 400x the rest of the workspace.  A plane the handle holds is given
// up only once its larger successor is in hand.  A size that was refused is remembered so that a serving loop does not pay a
// failing hipMalloc (and its device synchronisation) per call; the refusal expires after kRefusalAsks solves that wanted it.
constexpr int kRefusalAsks = 64;
void* ensure_plane(gclm_handle* h, gclm_handle::ScratchPlane& pl, size_t bytes) {
    if (bytes == 0) return nullptr;
    if (bytes <= pl.bytes) return pl.buf;
    if (pl.refused && bytes >= pl.refused) {
        if (++pl.refused_asks < kRefusalAsks) return nullptr;
        pl.refused = 0;                       // expired: this solve asks again
    }
    auto refuse = [&]() -> void* { pl.refused = bytes; pl.refused_asks = 0; return nullptr; };     // (the old, smaller plane stays)
    if (h->slat_limit && bytes > h->slat_limit) return refuse();
    if (!h->slat_limit) {                     // built-in rule: half of what is free once the old plane is released
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > (free_b + pl.bytes) / 2) {
            (void)hipGetLastError();
            return refuse();
        }
    }
    void* p = nullptr;
    const bool ok = hipMalloc(&p, bytes) == hipSuccess && p != nullptr;
    if (!ok) {
        (void)hipGetLastError();          // the failure is handled here: it must not surface in the next launch's status
        return refuse();
    }
    if (pl.buf) (void)hipFree(pl.buf);
    pl.buf = p;
    pl.bytes = bytes;
    return pl.buf;
}

int timed_sweep(gclm_handle* h, const SweepArgs& a, hipStream_t s, const FusedArgs* fused = nullptr) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool timing = h->timing && h->ev_used < 2 * 8192;   // bounded: stop recording silently
    if (timing) {
        while ((int)h->ev.size() < h->ev_used + 2) {
            hipEvent_t e;
            GCLM_HIP(h, hipEventCreate(&e));
            h->ev.push_back(e);
        }
        e0 = h->ev[h->ev_used];
        e1 = h->ev[h->ev_used + 1];
        h->ev_used += 2;
        GCLM_HIP(h, hipEventRecord(e0, s));
    }
    if (fused) GCLM_HIP(h, launch_fused_step(h->cfg.camera_model, a, *fused, s));
    else GCLM_HIP(h, launch_sweep(h->cfg.camera_model, a, s));
    if (timing) GCLM_HIP(h, hipEventRecord(e1, s));
    return 0;
}

int check_shapes(gclm_handle* h, const float* lat, int B, int H, int W) {
    // (an EMPTY batch has no fields: a zero-size device tensor's pointer is NULL -- solve_empty_shard)
    if (!lat && B != 0) return fail(h, -3, "latitude_field is required (lm_optimizer.py:31 raises KeyError without it)");
    if (B < 0 || H <= 0 || W <= 0) return fail(h, -3, "bad shape B=%d H=%d W=%d", B, H, W);
    if (B > kMaxCallImages) return fail(h, -3, "batch %d exceeds %d images per call (grid.y): split the batch", B, kMaxCallImages);
    if ((size_t)H * W >= (size_t)1 << 30) return fail(h, -3, "image too large");
    return 0;
}

int setup_groups(gclm_handle* h, int B) {
    SolveCtx& c = h->ctx;
    c.group_of_frame = nullptr;
    if (!h->cfg.shared_intrinsics) { c.n_groups = 0; c.group_size = 1; return 0; }
    const int gs = h->cfg.group_size > 0 ? h->cfg.group_size : (B > 0 ? B : 1);
    if (B % gs != 0) return fail(h, -3, "batch %d is not a multiple of group_size %d", B, gs);
    c.group_size = gs;
    c.n_groups = B / gs;
    return 0;
}

// How this call's sweeps walk the image, as ONE decision: one launch per LM step | row pairs | the one-row walk.
//  * One launch per LM step (gclm_pass.hip: fused_step_kernel) pays when a step is bound by its two dependent launches
//    rather than by the sweep: few workgroups in flight (GCLM_FUSED_MAX_WORKGROUPS).  It is VALID when the early-stop
//    decision is local to a workgroup (one image) or off, for independent intrinsics on the float4 path.
//  * Row pairs (gclm_pass.hip: row_math_mirror): radial / simple_divisional on the five-plane float4 sweep over an even
//    number of rows; never the one-launch-per-step path (its geometry, its prefetch).
void Plan::choose_walk(const gclm_handle* h, int B, int H, int W, bool aligned16, bool five) {
    const gclm_config& c = h->cfg;
    geo = plan_geometry(B, H, W, aligned16, h->sweep_iters, c.camera_model);
    const bool few = (long long)B * geo.nchunks <= GCLM_FUSED_MAX_WORKGROUPS;
    const bool fusable = !c.shared_intrinsics && geo.vec == 4 && (B == 1 || !c.early_stop) && B > 0 &&
                         !(c.early_stop && h->stop_comm);       // a stop that spans ranks is never local to a workgroup
    const bool pairable = geo.vec == 4 && five && !(H & 1) && H >= 4 &&
                          (h->row_pairs > 0 ? sweep_has_mirror(c.camera_model) : sweep_mirror_builtin(c.camera_model));
    bool pairs = false;
    if (pairable && h->row_pairs < 0) {
        // built-in choice: only launches too large for one launch per step, WHETHER OR NOT that path is valid for the call
        // (early stop over several images, gclm_set_fused_steps(h, 0)): below the threshold a step is latency-bound, and the
        // two-launch sequence stays the one-launch path's twin bit for bit
        pairs = !few;
    } else if (pairable && h->row_pairs > 0) {
        pairs = !(h->fused_mode == 1 && fusable);    // asked for both: the step that can be ONE launch stays one launch
    }
    one_launch = !pairs && fusable && (h->fused_mode == 1 || (h->fused_mode < 0 && few));
    if (pairs) geo = plan_geometry(B, H, W, aligned16, h->sweep_iters, c.camera_model, true);
}

// Would a call of `pixels` pixels that runs `sweeps` sweeps on plan `p` keep its confidences packed, the handle's mode and the
// kernels permitting?  (make_plan, which also knows the call's other planes, and gclm_plan_conf_pack.)
bool wants_conf_pack(const gclm_handle* h, const Plan& p, bool five, int sweeps, long long pixels) {
    const int model = h->cfg.camera_model;
    return model == GCLM_PINHOLE && p.geo.vec == 4 && five && !p.one_launch && sweeps >= 2 && h->conf_pack != 0 &&
           sweep_has_conf_pack(model) && (h->conf_pack > 0 || (pixels >= GCLM_CONF_PACK_MIN_PIXELS && sweeps >= 6));
}

// The one preamble of gclm_solve / gclm_calibrate, gclm_system and gclm_shared_begin: the plan of a call that runs `sweeps`
// sweeps over fields `f` of B images (0: an empty shard of a session, planned as one image), the sizes in h->ctx and the
// workspace.  The caller has set the group fields and iso_final of h->ctx.  `sin_lat`: the plane the caller handed, or null.
int make_plan(gclm_handle* h, Plan& p, const Fields& f, int B, int H, int W, const float* sin_lat, int sweeps,
              bool may_pack = true) {
    const int Bp = B > 0 ? B : 1, model = h->cfg.camera_model;
    p = Plan{};
    p.f = f;
    p.choose_walk(h, Bp, H, W, f.aligned16(), f.five());
    SolveCtx& c = h->ctx;
    c.cfg = h->cfg;
    c.B = B; c.H = H; c.W = W; c.nchunks = p.geo.nchunks;
    const bool float4_five = p.geo.vec == 4 && f.five();
    // The plane of sin(latitude_field) a caller handed (gclm_solve_ex, gclm_calibrate_ex, gclm_shared_begin_ex) that this
    // solve's sweeps read in place of `lat`, from the first sweep on -- or null: they read the radians, as without the plane.
    // Read by the five-plane float4 sweeps of the distortion models (one-row and row-pair walks) and by the five-plane
    // one-launch-per-step kernel of every model; ignored by pinhole's batch sweeps (memory-bound: the review keeps that kernel
    // as it is), the scalar path, four-plane and latitude-only sweeps, and a plane whose 16-byte alignment differs from the
    // other planes' (include/gclm.h says so).  Such a solve never wants the library's own plane.
    if (sin_lat && float4_five && is_aligned(sin_lat, 16) && (p.one_launch || model != GCLM_PINHOLE)) p.given = sin_lat;
    // Does this solve keep sin(latitude_field) in a scratch plane of its own (gclm_pass.hip: row_math, SLAT)?  Built-in choice:
    // the VALU-bound distortion models, on the five-plane float4 sweep, whenever at least one loop sweep precedes the final one.
    // Pinhole never (memory-bound: the plane's extra write costs what the saved arithmetic gains); not the one-launch-per-step
    // path (latency-bound, a handful of workgroups).
    const bool keep = !p.given && h->slat_plane != 0 && !p.one_launch && float4_five && sweeps >= 2 &&
                      !(h->slat_plane < 0 && model == GCLM_PINHOLE) && sweep_has_slat_plane(model);
    if (int rc = ensure_workspace(h, Bp, p.geo.nchunks, c.n_groups)) return rc;
    p.slat = static_cast<float*>(ensure_plane(h, h->slat, keep ? (size_t)B * H * W * sizeof(float) : 0));
    // Does it keep its two confidence planes as one plane of packed words (gclm_pass.hip: row_math, CPACK)?  Pinhole's batch
    // sweeps only (memory-bound: 16 instead of 20 bytes per pixel from the second sweep on), never beside another plane, not a
    // split shared-intrinsics session (`may_pack`).  Built-in choice: large calls (GCLM_CONF_PACK_MIN_PIXELS, 874 images of
    // 640x480: the plane pays from 110 images on, profiles/conf_pack_crossover.json, but below the threshold a sweep's launch
    // time over the caller's five planes stays a true HBM rate, which the benchmark's records of such batches state) that are
    // long enough to pay for the fill, which costs about three later sweeps' saving (wants_conf_pack).
    const long long pixels = (long long)B * H * W;
    const bool pack = may_pack && !p.given && !p.slat && wants_conf_pack(h, p, f.five(), sweeps, pixels);
    p.cpack = static_cast<uint32_t*>(ensure_plane(h, h->cpack, pack ? (size_t)pixels * sizeof(uint32_t) : 0));
    h->cpack_images = p.cpack ? B : 0;
    h->sh.active = false;
    return 0;
}

// The arguments of the plan's next sweep with parameter blocks `pb`.  A solve that reads the caller's plane: every sweep
// loads it (SLAT = 2); one that keeps a scratch plane (sin(latitude), or the packed confidences): the first sweep fills it,
// the others read it.
SweepArgs Plan::next_sweep(const gclm_handle* h, const PBlock* pb, bool loop_params, int stop_step) {
    SweepArgs a{};
    a.up = f.up; a.lat = f.lat; a.upc = f.up ? f.upc : nullptr; a.latc = f.latc;
    a.pb = pb; a.ctrl = h->ctx.ctrl; a.partials = h->ctx.partials;
    a.B = h->ctx.B; a.H = h->ctx.H; a.W = h->ctx.W;
    a.nchunks = geo.nchunks; a.vec = geo.vec;
    a.wu = geo.wu; a.cu = geo.cu; a.nstrips = geo.nstrips; a.rpi = geo.rpi; a.rows_per_block = geo.rows_per_block; a.wpt = geo.wpt; a.jobs = geo.jobs;
    a.hrows = geo.hrows; a.mirror = geo.mirror;
    // loop sweeps: the configured parametrisation; final sweep: the (roll, pitch, focal) block, in its log-focal form when
    // every image is known to have fx == fy (iso_final: finalize_kernel rescales the focal column)
    a.log_focal = loop_params ? h->cfg.use_log_focal : h->ctx.iso_final;
    a.stop_step = stop_step;
    a.up_scale = h->cfg.up_loss_fn_scale; a.lat_scale = h->cfg.lat_loss_fn_scale;
    if (given) {
        a.slat = const_cast<float*>(given);     // (slat_mode 2 never writes through it)
        a.lat = given;
        a.slat_mode = 2;
    } else if (slat) {
        a.slat = slat;
        if (slat_filled) a.lat = slat;
        a.slat_mode = slat_filled ? 2 : 1;
        slat_filled = true;
    }
    if (cpack) {
        a.cpack = cpack;
        a.cpack_flags = h->ctx.cpack_flags;
        a.cpack_mode = cpack_filled ? 2 : 1;
        cpack_filled = true;
    }
    return a;
}

// Paced launches (single image with early stop): the launches after the stop are skipped on the device, but each
// still costs its turn on the queue (2.3 us x 21 of a default-conf solve).  Launch k is therefore only issued
// once launch k - depth has reported (a word in host-mapped memory), and none once the stop is reported.  What
// the host sees only decides how many launches it issues: the device-side skip stays in force, so a late or
// missing report costs time, never correctness; the wait is bounded (kPacedPatienceUs, then a cool-down).
struct Pacer {
    gclm_handle* h;
    bool paced;                 // the launches of this solve report (FusedArgs::progress) ...
    bool waiting;               // ... and the host still waits for them
    bool stop_seen = false;     // a report said that the early stop fired: no further loop launch is issued

    // begin a solve: a new epoch in the progress word, unless the handle is cooling down after a wait that timed out
    Pacer(gclm_handle* handle, bool single_image_early_stop)
        : h(handle), paced(handle->paced_depth > 0 && single_image_early_stop && handle->progress_host) {
        if (paced && h->paced_cooldown > 0) { --h->paced_cooldown; paced = false; }
        if (paced) h->epoch = (h->epoch + 1) & kPacedEpochMask;
        waiting = paced;
    }
    bool reported(int launch) {          // has `launch` (or a later one) of THIS solve reported?  sets stop_seen
        const unsigned v = __atomic_load_n(h->progress_host, __ATOMIC_ACQUIRE);
        if (((v >> kPacedEpochShift) & kPacedEpochMask) != h->epoch) return false;
        if (v & kPacedStopBit) stop_seen = true;
        return stop_seen || (v & 0xffffu) >= (unsigned)(launch + 1);
    }
    // before loop launch `step` is issued: wait for launch step - depth.
    // A launch of this solve reports within a few microseconds of the previous one when the queue is ours.
    // Spin briefly (the common case), then yield the core between polls; give up after kPacedPatienceUs.
    // A queue backed up by other streams (a serving loop overlapping the CNN with the LM) trips that: the rest
    // of THIS solve is issued unpaced, and the handle stops pacing for the next kPacedCooldown solves instead
    // of burning the patience on every call.
    void wait_before(int step) {
        if (!waiting || step < h->paced_depth) return;
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spin = 0; !reported(step - h->paced_depth); ++spin) {
            if (spin < 256) continue;
            std::this_thread::yield();
            if ((spin & 0xf) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(kPacedPatienceUs)) {
                waiting = false;
                h->paced_cooldown = kPacedCooldown;
                break;
            }
        }
    }
};

// an empty shard still owes its peers the per-step collectives of a rank-spanning early stop (zero counters)
int solve_empty_shard(gclm_handle* h, int H, int W, const InitArgs& ia, hipStream_t s) {
    if (!(h->cfg.early_stop && h->stop_comm && h->cfg.num_steps > 1)) return 0;
    DeviceGuard guard(h->device);
    GCLM_HIP(h, guard.status);
    SolveCtx& c = h->ctx;
    c.cfg = h->cfg;
    c.B = 0; c.H = H; c.W = W; c.nchunks = 1; c.n_groups = 0; c.group_size = 1; c.group_of_frame = nullptr;
    if (int rc = ensure_workspace(h, 1, 1, 0)) return rc;
    GCLM_HIP(h, launch_init(c, ia, s));                               // thread 0 resets the counters
    for (int step = 1; step < h->cfg.num_steps; ++step)
        if (gclm_comm_all_reduce_sum_i32(h->stop_comm, &c.ctrl->notclose[step], 1, s) != 0)
            return fail(h, -20, "early-stop all-reduce failed: %s", gclm_comm_last_error(h->stop_comm));
    return 0;
}

// fused(step) x num_steps | fused(final) | finalize : num_steps + 2 launches, partial records double-buffered
// (the first launch builds theta_0 itself: no init launch)
int solve_one_launch_per_step(gclm_handle* h, Plan& p, const InitArgs& ia, float* d_cam_out, float* d_grav_out,
                              float* d_info_out, hipStream_t s) {
    const SolveCtx& c = h->ctx;
    float* const part[2] = {c.partials, c.partials2};
    Pacer pacer(h, h->cfg.early_stop && c.B == 1);
    for (int step = 0; step <= h->cfg.num_steps; ++step) {
        const bool fin = step == h->cfg.num_steps;
        if (!fin) pacer.wait_before(step);
        if (pacer.stop_seen && !fin) continue;       // the final launch finds the stop in the counters, as it always does
        SweepArgs a = p.next_sweep(h, c.pb[0], !fin, 0);        // (never the library's plane here: make_plan)
        a.partials = part[step & 1];
        FusedArgs f;
        f.c = c;
        f.step = step;
        f.is_final = fin ? 1 : 0;
        f.partials_in = part[(step + 1) & 1];
        f.progress = (pacer.paced && !fin) ? h->progress_dev : nullptr;
        f.epoch = h->epoch;
        f.ia = ia;
        f.init_here = step == 0 ? 1 : 0;
        if (int rc = timed_sweep(h, a, s, &f)) return rc;
    }
    SolveCtx cf = c;
    cf.partials = part[h->cfg.num_steps & 1];        // the final sweep's records
    GCLM_HIP(h, launch_finalize(cf, d_cam_out, d_grav_out, d_info_out, s));
    return 0;
}

// init | { sweep(theta_i) ; update_i } x num_steps | prep_final ; sweep(theta_final, rpf) ; finalize
int solve_two_launches_per_step(gclm_handle* h, Plan& p, const InitArgs& ia, float* d_cam_out, float* d_grav_out,
                                float* d_info_out, hipStream_t s, float* d_record = nullptr, const SoftPrior& sp = SoftPrior{}) {
    const SolveCtx& c = h->ctx;
    const bool es = h->cfg.early_stop != 0;
    GCLM_HIP(h, launch_init(c, ia, s));
    for (int step = 0; step < h->cfg.num_steps; ++step) {
        if (int rc = timed_sweep(h, p.next_sweep(h, c.pb[step & 1], true, es ? step : 0), s)) return rc;
        if (!h->cfg.shared_intrinsics) {
            GCLM_HIP(h, launch_update(c, step, s, d_record, sp));
        } else {
            GCLM_HIP(h, launch_shared_step(c, step, s));     // reduce + Schur solve + update: one launch
        }
        // a batch sharded over ranks: "whose cost still moved" is a count over ALL ranks' images (every step, also after
        // the stop -- the counters of skipped steps stay 0 everywhere -- so that the ranks' collectives keep matching)
        if (es && h->stop_comm && step >= 1)
            if (gclm_comm_all_reduce_sum_i32(h->stop_comm, &c.ctrl->notclose[step], 1, s) != 0)
                return fail(h, -20, "early-stop all-reduce failed: %s", gclm_comm_last_error(h->stop_comm));
    }
    GCLM_HIP(h, launch_prep_final(c, s));
    if (int rc = timed_sweep(h, p.next_sweep(h, c.pb_final, false, 0), s)) return rc;
    GCLM_HIP(h, launch_finalize(c, d_cam_out, d_grav_out, d_info_out, s, sp));
    return 0;
}

// `soft`: the soft priors of gclm_calibrate_soft (all null elsewhere); soft.cost null: the handle's own (B,2) floats
int run_solve(gclm_handle* h, const Fields& f, int B, int H, int W, const InitArgs& ia, float* d_cam_out,
              float* d_grav_out, float* d_info_out, const float* d_sin_lat, void* stream, float* d_record = nullptr,
              SoftPrior soft = SoftPrior{}) {
    if (int rc = check_shapes(h, f.lat, B, H, W)) return rc;
    if (d_record && h->cfg.shared_intrinsics) return fail(h, -3, "the step record is kept for per-image solves only");
    if (soft.on() && h->cfg.shared_intrinsics) return fail(h, -3, "soft priors are for per-image solves only");
    if (soft.on() && !(h->cfg.use_spherical_manifold && h->cfg.use_log_focal))
        return fail(h, -3, "soft priors need use_spherical_manifold and use_log_focal");
    if (B > 0 && (!d_cam_out || !d_grav_out || !d_info_out)) return fail(h, -3, "null output pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    h->sh.active = false;       // any solve ends a split session, also the empty one, which plans nothing (make_plan does it for the others)
    if (B == 0) return solve_empty_shard(h, H, W, ia, s);
    DeviceGuard guard(h->device);
    GCLM_HIP(h, guard.status);
    if (int rc = setup_groups(h, B)) return rc;
    // trivial / heuristic initial estimate without `scales`: fx == fy at the start, and update_focal keeps the ratio
    // (camera.py:148) -- the final sweep may then run the cheaper log-focal instantiation (see finalize_kernel)
    h->ctx.iso_final = (ia.cam == nullptr && ia.scales == nullptr && GCLM_ISO_FINAL) ? 1 : 0;
    Plan p;
    if (int rc = make_plan(h, p, f, B, H, W, d_sin_lat, h->cfg.num_steps + 1)) return rc;
    if (soft.on() && !soft.cost) soft.cost = h->prior_cost;
    if (d_record || soft.on()) {
        // the record is written, and the soft priors are added, by the per-image update kernel: a call planned as one launch
        // per step takes its two-launch twin (same geometry, no plane of its own: the plan above stands), which computes the
        // same bits
        p.one_launch = false;
        if (d_record) GCLM_HIP(h, hipMemsetAsync(d_record, 0, sizeof(float) * GCLM_LM_RECORD_STRIDE * (size_t)B * h->cfg.num_steps, s));
        // (num_steps = 0: no update writes the initial prior cost, which is then the final one's slot neighbour: zero it)
        if (soft.on() && h->cfg.num_steps == 0) GCLM_HIP(h, hipMemsetAsync(soft.cost, 0, sizeof(float) * 2 * (size_t)B, s));
        return solve_two_launches_per_step(h, p, ia, d_cam_out, d_grav_out, d_info_out, s, d_record, soft);
    }
    if (p.one_launch) return solve_one_launch_per_step(h, p, ia, d_cam_out, d_grav_out, d_info_out, s);
    return solve_two_launches_per_step(h, p, ia, d_cam_out, d_grav_out, d_info_out, s);
}

}  // namespace

namespace gclm {
// Cut one sweep into column-stationary tiles and wave jobs (gclm_pass.hip: sweep_kernel).  A row holds `wu` units
// (float4 groups, or pixels in the scalar path).  Up to 512 units per row the strip is the whole row and a tile takes
// `rpi` rows per iteration with rpi * wu lanes rounded up to whole waves -- rpi is chosen for the fewest idle lanes,
// then for the smallest tile (640 px: 160 units, rpi = 2, 320 lanes = 5 waves, no idle lane).  Wider rows are cut
// into strips of a multiple of 64 units, one row per iteration.  Every wave of a tile is a job; a workgroup is four
// consecutive jobs of an image.
Geometry plan_geometry(int B, int H, int W, bool aligned16, int sweep_iters, int camera_model, bool mirror) {
    Geometry g;
    g.vec = (aligned16 && (W % 4 == 0)) ? 4 : 1;
    // row pairs (gclm_pass.hip: row_math_mirror): the tiles walk rows [0, H / 2), every lane takes row H - y along with row y
    g.mirror = (mirror && g.vec == 4 && H % 2 == 0 && H >= 4) ? 1 : 0;
    g.hrows = g.mirror ? H / 2 : H;
    const int rows = g.hrows;
    g.wu = W / g.vec;
    auto waste = [](int used, int lanes) { return (int)(50.0 * (lanes - used) / lanes); };   // idle lanes, steps of 2 %
    if (g.wu <= kMaxTile) {
        g.nstrips = 1;
        g.cu = g.wu;
        g.rpi = 1;
        int best = 1 << 30;
        for (int r = 1; r * g.wu <= kMaxTile; ++r) {
            const int lanes = (r * g.wu + 63) / 64 * 64;
            const int score = waste(r * g.wu, lanes) * 1024 + lanes / 64;
            if (score < best) { best = score; g.rpi = r; }
        }
        g.wpt = (g.rpi * g.wu + 63) / 64;
    } else {
        g.rpi = 1;
        g.cu = 256;
        int best = 1 << 30;
        for (int cu = 128; cu <= kMaxTile; cu += 64) {
            const int ns = (g.wu + cu - 1) / cu;
            const int score = waste(g.wu, ns * cu) * 1024 + cu / 64;
            if (score < best) { best = score; g.cu = cu; }
        }
        g.nstrips = (g.wu + g.cu - 1) / g.cu;
        g.wpt = g.cu / 64;
    }
    // ~20 loop iterations per lane amortise the 16-value workgroup reduction; fewer when the batch alone cannot
    // fill 256 CUs x 4+ workgroups.
    // The distortion models are VALU-bound: their per-workgroup prologue / epilogue is worth amortising over
    // 30 iterations where the image divides into whole blocks of that many rows (640x480: 8 blocks of 60 rows; same-allocation
    // A/B profiles/archive/r04_variant_huber_clamp.log: simple_radial -0.3 %, radial -1.2 %, simple_divisional -0.7 %, pinhole +0.4 %).
    // Row pairs: an iteration is two rows of the image -- half the iterations for the same work per workgroup.
    int builtin = g.mirror ? 10 : 20;
    if (camera_model != GCLM_PINHOLE && rows % (g.rpi * (g.mirror ? 15 : 30)) == 0) builtin = g.mirror ? 15 : 30;
    int iters = (sweep_iters >= 1 && sweep_iters <= 4096) ? sweep_iters : builtin;   // gclm_set_sweep_iters (tuning / tests)
    auto jobs = [&](int it) { return g.nstrips * g.wpt * ((rows + g.rpi * it - 1) / (g.rpi * it)); };
    auto chunks = [&](int it) { return (jobs(it) + kBlock / 64 - 1) / (kBlock / 64); };
    while (iters > 2 && (long long)B * chunks(iters) < 2048) iters = iters > 5 ? iters / 2 : iters - 1;
    g.rows_per_block = g.rpi * iters;
    g.jobs = jobs(iters);
    g.nchunks = chunks(iters);
    return g;
}
}  // namespace gclm

extern "C" {

int gclm_version(void) { return GCLM_VERSION; }

int gclm_abi_config_size(void) { return (int)sizeof(gclm_config); }

int gclm_default_config(gclm_config* cfg) {
    if (!cfg) return -1;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(gclm_config);
    cfg->abi_version = GCLM_VERSION;
    cfg->device = 0;
    cfg->camera_model = GCLM_PINHOLE;
    cfg->num_steps = 30;
    cfg->lambda0 = 0.1f;
    cfg->early_stop = 1;
    cfg->atol = 1e-8f;
    cfg->rtol = 1e-8f;
    cfg->use_spherical_manifold = 1;
    cfg->use_log_focal = 1;
    cfg->up_loss_fn_scale = 1e-2f;
    cfg->lat_loss_fn_scale = 1e-2f;
    cfg->estimate_gravity = cfg->estimate_focal = cfg->estimate_dist = 1;
    cfg->compute_uncertainty = 1;
    return 0;
}

int gclm_create(gclm_handle** out, const gclm_config* cfg) {
    if (!out || !cfg) return fail(nullptr, -1, "gclm_create: null argument");
    *out = nullptr;
    char abuf[256];
    if (const char* msg = abi_mismatch(cfg, abuf)) return fail(nullptr, -5, "gclm_create: %s", msg);
    if (const char* msg = validate(*cfg)) return fail(nullptr, -2, "gclm_create: %s", msg);
    const int device = cfg->device;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, -11, "gclm_create: no HIP device visible (the HIP path has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, -2, "gclm_create: device %d out of range (%d devices)", device, ndev);
    gclm_handle* h = new (std::nothrow) gclm_handle();
    if (!h) return fail(nullptr, -12, "gclm_create: out of host memory");
    h->cfg = *cfg;
    h->device = device;
    *out = h;
    return 0;
}

int gclm_configure(gclm_handle* h, const gclm_config* cfg) {
    if (!h || !cfg) return -1;
    char abuf[256];
    if (const char* msg = abi_mismatch(cfg, abuf)) return fail(h, -5, "gclm_configure: %s", msg);
    if (const char* msg = validate(*cfg)) return fail(h, -2, "gclm_configure: %s", msg);
    if (cfg->device != h->device) return fail(h, -2, "gclm_configure: a handle cannot move from device %d to %d", h->device, (int)cfg->device);
    h->cfg = *cfg;
    h->sh.active = false;
    return 0;
}

int gclm_destroy(gclm_handle* h) {
    if (!h) return 0;
    DeviceGuard guard(h->device);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    if (h->ws) (void)hipFree(h->ws);
    if (h->slat.buf) (void)hipFree(h->slat.buf);
    if (h->cpack.buf) (void)hipFree(h->cpack.buf);
    if (h->progress_host) (void)hipHostFree(h->progress_host);
    delete h;
    return 0;
}

const char* gclm_last_error(const gclm_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

size_t gclm_workspace_bytes(const gclm_handle* h) { return h ? h->ws_bytes + h->slat.bytes + h->cpack.bytes : 0; }

size_t gclm_slat_plane_bytes(const gclm_handle* h) { return h ? h->slat.bytes : 0; }

size_t gclm_conf_pack_bytes(const gclm_handle* h) { return h ? h->cpack.bytes : 0; }

int gclm_set_slat_plane_limit(gclm_handle* h, size_t max_bytes) {
    if (!h) return -1;
    h->slat_limit = max_bytes;
    h->slat.refused = h->cpack.refused = 0;
    h->sh.active = false;
    return 0;
}

int gclm_release_workspace(gclm_handle* h) {
    if (!h) return -1;
    DeviceGuard guard(h->device);
    GCLM_HIP(h, guard.status);
    h->sh.active = false;
    if (h->ws) GCLM_HIP(h, hipFree(h->ws));                // (hipFree waits for the device: nothing of this handle is in flight after)
    h->ws = nullptr;
    h->ws_bytes = 0;
    h->ctx = SolveCtx{};
    h->group_partials = nullptr;
    for (gclm_handle::ScratchPlane* pl : {&h->slat, &h->cpack}) {
        if (pl->buf) GCLM_HIP(h, hipFree(pl->buf));
        *pl = gclm_handle::ScratchPlane{};
    }
    h->cpack_images = 0;
    return 0;
}

int gclm_set_sweep_iters(gclm_handle* h, int iters) {
    if (!h) return -1;
    if (iters < 0 || iters > 4096) return fail(h, -3, "gclm_set_sweep_iters: %d out of range [0, 4096]", iters);
    h->sweep_iters = iters;
    h->sh.active = false;
    return 0;
}

int gclm_plan_cut(const gclm_handle* h, int B, int H, int W, int aligned16, int* rows_per_chunk, int* chunks_per_image) {
    if (!h) return -1;
    if (B < 1 || H < 1 || W < 1) return -3;
    Plan p;
    p.choose_walk(h, B, H, W, aligned16 != 0, true);       // (as for the five planes of a complete field set)
    if (rows_per_chunk) *rows_per_chunk = p.geo.rows_per_block;
    if (chunks_per_image) *chunks_per_image = p.geo.nchunks;
    return 0;
}

int gclm_plan_conf_pack(const gclm_handle* h, int B, int H, int W, int aligned16, int five_planes, int sweeps, int* pack) {
    if (!h || !pack) return -1;
    if (B < 1 || H < 1 || W < 1) return -3;
    Plan p;
    p.choose_walk(h, B, H, W, aligned16 != 0, five_planes != 0);
    *pack = wants_conf_pack(h, p, five_planes != 0, sweeps, (long long)B * H * W) ? 1 : 0;
    return 0;
}

int gclm_set_slat_plane(gclm_handle* h, int mode) {
    if (!h) return -1;
    if (mode < -1 || mode > 1) return fail(h, -3, "gclm_set_slat_plane: mode %d not in {-1, 0, 1}", mode);
    h->slat_plane = mode;
    h->slat.refused = 0;
    h->sh.active = false;
    return 0;
}

int gclm_set_conf_pack(gclm_handle* h, int mode) {
    if (!h) return -1;
    if (mode < -1 || mode > 1) return fail(h, -3, "gclm_set_conf_pack: mode %d not in {-1, 0, 1}", mode);
    h->conf_pack = mode;
    h->cpack.refused = 0;
    return 0;
}

int gclm_conf_pack_fallbacks(gclm_handle* h, int* n) {
    if (!h || !n) return -1;
    *n = 0;
    if (h->cpack_images == 0 || !h->ctx.cpack_flags) return 0;
    DeviceGuard guard(h->device);
    GCLM_HIP(h, guard.status);
    GCLM_HIP(h, hipDeviceSynchronize());
    std::vector<unsigned> flags(h->cpack_images);
    GCLM_HIP(h, hipMemcpy(flags.data(), h->ctx.cpack_flags, flags.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (unsigned f : flags) *n += f != 0;
    return 0;
}

int gclm_set_row_pairs(gclm_handle* h, int mode) {
    if (!h) return -1;
    if (mode < -1 || mode > 1) return fail(h, -3, "gclm_set_row_pairs: mode %d not in {-1, 0, 1}", mode);
    h->row_pairs = mode;
    h->sh.active = false;
    return 0;
}

int gclm_set_stop_comm(gclm_handle* h, gclm_comm* c) {
    if (!h) return -1;
    h->stop_comm = c;
    return 0;
}

int gclm_merge_stop_at(gclm_handle* const* parts, float* const* d_info, const int* B, int n_parts, void* stream) {
    if (!parts || !d_info || !B || n_parts < 1 || !parts[0]) return -1;
    gclm_handle* h0 = parts[0];
    if (n_parts > kMaxMergeParts) return fail(h0, -3, "gclm_merge_stop_at: %d parts, at most %d", n_parts, kMaxMergeParts);
    MergeStopArgs a{};
    a.n = 0;
    a.num_steps = h0->cfg.num_steps;
    for (int p = 0; p < n_parts; ++p) {
        gclm_handle* h = parts[p];
        if (B[p] < 0) return fail(h0, -3, "gclm_merge_stop_at: part %d has a negative size", p);
        // an EMPTY part holds no image: it adds nothing to the counters and has no row to write (its handle may never have
        // solved anything, or may hold the counters of an older, non-empty solve -- a B = 0 solve does not touch them)
        if (B[p] == 0) continue;
        if (!h || !h->ctx.ctrl || !d_info[p]) return fail(h0, -3, "gclm_merge_stop_at: part %d has not solved anything", p);
        if (h->device != h0->device || h->cfg.num_steps != h0->cfg.num_steps || h->cfg.early_stop)
            return fail(h0, -2, "gclm_merge_stop_at: the parts must share device and num_steps and run with early_stop = 0");
        if (B[p] != h->ctx.B)       // the counters in this handle's workspace are those of its LAST solve
            return fail(h0, -2, "gclm_merge_stop_at: part %d is given as %d images, but the last solve of its handle had %d", p, B[p],
                        h->ctx.B);
        a.ctrl[a.n] = h->ctx.ctrl;
        a.info[a.n] = d_info[p];
        a.B[a.n] = B[p];
        ++a.n;
    }
    if (a.n == 0) return 0;
    DeviceGuard guard(h0->device);
    GCLM_HIP(h0, guard.status);
    GCLM_HIP(h0, launch_merge_stop(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int gclm_set_fused_steps(gclm_handle* h, int mode) {
    if (!h) return -1;
    if (mode < -1 || mode > 1) return fail(h, -3, "gclm_set_fused_steps: mode %d not in {-1, 0, 1}", mode);
    h->fused_mode = mode;
    return 0;
}

int gclm_set_paced_launches(gclm_handle* h, int depth) {
    if (!h) return -1;
    if (depth < 0 || depth > 16) return fail(h, -3, "gclm_set_paced_launches: depth %d out of range [0, 16]", depth);
    if (depth > 0 && !h->progress_host) {
        DeviceGuard guard(h->device);
        GCLM_HIP(h, guard.status);
        void* p = nullptr;
        GCLM_HIP(h, hipHostMalloc(&p, 64, hipHostMallocMapped));
        h->progress_host = static_cast<unsigned*>(p);
        *h->progress_host = 0;
        void* d = nullptr;
        GCLM_HIP(h, hipHostGetDevicePointer(&d, p, 0));
        h->progress_dev = static_cast<unsigned*>(d);
    }
    h->paced_depth = depth;
    return 0;
}

int gclm_set_timing(gclm_handle* h, int enabled) {
    if (!h) return -1;
    h->timing = enabled != 0;
    h->ev_used = 0;
    return 0;
}

int gclm_last_pass_timing(gclm_handle* h, int* n_launches, float* total_ms) {
    if (!h) return -1;
    if (!h->timing) return fail(h, -4, "timing not enabled");
    float tot = 0.f;
    for (int i = 0; i + 1 < h->ev_used; i += 2) {
        GCLM_HIP(h, hipEventSynchronize(h->ev[i + 1]));
        float ms = 0.f;
        GCLM_HIP(h, hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
        tot += ms;
    }
    if (n_launches) *n_launches = h->ev_used / 2;
    if (total_ms) *total_ms = tot;
    h->ev_used = 0;          // events accumulate over solves until read
    return 0;
}

static int solve_entry(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                       const float* d_lat_conf, int B, int H, int W, float* d_cam_io, float* d_grav_io,
                       float* d_info_out, const float* d_sin_lat, float* d_record, void* stream) {
    if (!h) return -1;
    InitArgs ia{};
    ia.cam = d_cam_io;
    ia.grav = d_grav_io;
    if (B != 0 && (!d_cam_io || !d_grav_io)) return fail(h, -3, "gclm_solve: null camera / gravity pointer");
    return run_solve(h, Fields{d_up, d_lat, d_up_conf, d_lat_conf}, B, H, W, ia, d_cam_io, d_grav_io, d_info_out, d_sin_lat, stream, d_record);
}

int gclm_solve_ex(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                  const float* d_lat_conf, int B, int H, int W, float* d_cam_io, float* d_grav_io,
                  float* d_info_out, const float* d_sin_lat, void* stream) {
    return solve_entry(h, d_up, d_lat, d_up_conf, d_lat_conf, B, H, W, d_cam_io, d_grav_io, d_info_out, d_sin_lat, nullptr, stream);
}

int gclm_solve_recorded(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                        const float* d_lat_conf, int B, int H, int W, float* d_cam_io, float* d_grav_io,
                        float* d_info_out, float* d_record, void* stream) {
    return solve_entry(h, d_up, d_lat, d_up_conf, d_lat_conf, B, H, W, d_cam_io, d_grav_io, d_info_out, nullptr, d_record, stream);
}

int gclm_solve(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
               const float* d_lat_conf, int B, int H, int W, float* d_cam_io, float* d_grav_io,
               float* d_info_out, void* stream) {
    return gclm_solve_ex(h, d_up, d_lat, d_up_conf, d_lat_conf, B, H, W, d_cam_io, d_grav_io, d_info_out, nullptr, stream);
}

static int calibrate_entry(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                           const float* d_lat_conf, int B, int H, int W, const float* d_scales,
                           const float* d_prior_focal, const float* d_prior_gravity, const float* d_prior_dist,
                           int prior_dist_cols, float* d_cam_out, float* d_grav_out, float* d_info_out,
                           const float* d_sin_lat, float* d_record, void* stream, const float* d_prior_focal_sigma = nullptr,
                           const float* d_prior_gravity_sigma = nullptr, float* d_prior_cost_out = nullptr) {
    if (!h) return -1;
    if (d_prior_dist && (prior_dist_cols < 1 || prior_dist_cols > 2)) return fail(h, -3, "gclm_calibrate: prior_dist_cols must be 1 or 2");
    // the free-parameter flags must agree with the priors (setup_optimization_and_priors, :204-221); an empty batch has
    // no prior rows either (NULL), and only takes part in the stop collectives
    // (a prior given with its standard deviation -- gclm_calibrate_soft -- keeps its column free)
    const bool hard_focal = d_prior_focal && !d_prior_focal_sigma, hard_gravity = d_prior_gravity && !d_prior_gravity_sigma;
    if (B != 0 && (hard_focal == (h->cfg.estimate_focal != 0) || hard_gravity == (h->cfg.estimate_gravity != 0)))
        return fail(h, -2, "gclm_calibrate: estimate_focal / estimate_gravity disagree with the priors passed");
    InitArgs ia{};
    ia.scales = d_scales;
    ia.prior_focal = d_prior_focal;
    ia.prior_gravity = d_prior_gravity;
    ia.prior_dist = d_prior_dist;
    ia.prior_dist_cols = prior_dist_cols;
    ia.up = d_up;
    ia.lat = d_lat;
    if (h->cfg.heuristic_init && !d_up && B != 0) return fail(h, -3, "gclm_calibrate: heuristic_init needs the up field");
    // (the initial estimate -- the heuristic one reads `lat` -- always reads the radians: ia.lat)
    SoftPrior soft{};
    if (d_prior_focal_sigma || d_prior_gravity_sigma) {
        soft.focal = d_prior_focal;
        soft.focal_sigma = d_prior_focal_sigma;
        soft.gravity = d_prior_gravity;
        soft.gravity_sigma = d_prior_gravity_sigma;
        soft.cost = d_prior_cost_out;
    }
    return run_solve(h, Fields{d_up, d_lat, d_up_conf, d_lat_conf}, B, H, W, ia, d_cam_out, d_grav_out, d_info_out, d_sin_lat, stream, d_record,
                     soft);
}

int gclm_calibrate_soft(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                        const float* d_lat_conf, int B, int H, int W, const float* d_scales,
                        const float* d_prior_focal, const float* d_prior_gravity, const float* d_prior_dist,
                        int prior_dist_cols, const float* d_prior_focal_sigma, const float* d_prior_gravity_sigma,
                        float* d_cam_out, float* d_grav_out, float* d_info_out, float* d_prior_cost_out,
                        const float* d_sin_lat, void* stream) {
    if (!d_prior_focal_sigma && !d_prior_gravity_sigma)         // gclm_calibrate_ex exactly; d_prior_cost_out is not written
        return calibrate_entry(h, d_up, d_lat, d_up_conf, d_lat_conf, B, H, W, d_scales, d_prior_focal, d_prior_gravity, d_prior_dist,
                               prior_dist_cols, d_cam_out, d_grav_out, d_info_out, d_sin_lat, nullptr, stream);
    // Everything that can be refused from the arguments alone comes first, before the handle is looked at and before any
    // HIP call (h == NULL: the message goes where gclm_create's does).
    if ((d_prior_focal_sigma && !d_prior_focal) || (d_prior_gravity_sigma && !d_prior_gravity))
        return fail(h, -3, "gclm_calibrate_soft: a standard deviation without its prior");
    if (B <= 0 || B > kMaxCallImages || H <= 0 || W <= 0) return fail(h, -3, "gclm_calibrate_soft: bad shape B=%d H=%d W=%d", B, H, W);
    if (!d_lat || !d_cam_out || !d_grav_out || !d_info_out) return fail(h, -3, "gclm_calibrate_soft: null field or output pointer");
    if (d_prior_dist && (prior_dist_cols < 1 || prior_dist_cols > 2)) return fail(h, -3, "gclm_calibrate_soft: prior_dist_cols must be 1 or 2");
    ArgCheck a;
    a.writes(d_cam_out, floats(B, GCLM_CAM_STRIDE), 4);
    a.writes(d_grav_out, floats(B, GCLM_GRAV_STRIDE), 4);
    a.writes(d_info_out, floats(B, GCLM_INFO_STRIDE), 4);
    a.writes(d_prior_cost_out, floats(B, 2), 4);
    a.reads(d_up, floats(B, 2, H, W), 4);
    a.reads(d_lat, floats(B, H, W), 4);
    a.reads(d_up_conf, floats(B, H, W), 4);
    a.reads(d_lat_conf, floats(B, H, W), 4);
    a.reads(d_sin_lat, floats(B, H, W), 4);
    a.reads(d_scales, floats(2), 4);
    a.reads(d_prior_focal, floats(B), 4);
    a.reads(d_prior_gravity, floats(B, 3), 4);
    a.reads(d_prior_dist, floats(B, prior_dist_cols > 0 ? prior_dist_cols : 1), 4);
    a.reads(d_prior_focal_sigma, floats(B), 4);
    a.reads(d_prior_gravity_sigma, floats(B), 4);
    if (!a.pass()) return fail(h, -3, "gclm_calibrate_soft: a misaligned pointer, or an output that overlaps another range of the call");
    if (!h) return -1;
    if (h->cfg.shared_intrinsics || !(h->cfg.use_spherical_manifold && h->cfg.use_log_focal))
        return fail(h, -3, "gclm_calibrate_soft: per-image solves on the spherical manifold and the log focal length only");
    return calibrate_entry(h, d_up, d_lat, d_up_conf, d_lat_conf, B, H, W, d_scales, d_prior_focal, d_prior_gravity, d_prior_dist,
                           prior_dist_cols, d_cam_out, d_grav_out, d_info_out, d_sin_lat, nullptr, stream, d_prior_focal_sigma,
                           d_prior_gravity_sigma, d_prior_cost_out);
}

int gclm_calibrate_ex(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                      const float* d_lat_conf, int B, int H, int W, const float* d_scales,
                      const float* d_prior_focal, const float* d_prior_gravity, const float* d_prior_dist,
                      int prior_dist_cols, float* d_cam_out, float* d_grav_out, float* d_info_out,
                      const float* d_sin_lat, void* stream) {
    return calibrate_entry(h, d_up, d_lat, d_up_conf, d_lat_conf, B, H, W, d_scales, d_prior_focal, d_prior_gravity, d_prior_dist,
                           prior_dist_cols, d_cam_out, d_grav_out, d_info_out, d_sin_lat, nullptr, stream);
}

int gclm_calibrate_recorded(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                            const float* d_lat_conf, int B, int H, int W, const float* d_scales,
                            const float* d_prior_focal, const float* d_prior_gravity, const float* d_prior_dist,
                            int prior_dist_cols, float* d_cam_out, float* d_grav_out, float* d_info_out,
                            float* d_record, void* stream) {
    return calibrate_entry(h, d_up, d_lat, d_up_conf, d_lat_conf, B, H, W, d_scales, d_prior_focal, d_prior_gravity, d_prior_dist,
                           prior_dist_cols, d_cam_out, d_grav_out, d_info_out, nullptr, d_record, stream);
}

int gclm_calibrate(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                   const float* d_lat_conf, int B, int H, int W, const float* d_scales,
                   const float* d_prior_focal, const float* d_prior_gravity, const float* d_prior_dist,
                   int prior_dist_cols, float* d_cam_out, float* d_grav_out, float* d_info_out, void* stream) {
    return gclm_calibrate_ex(h, d_up, d_lat, d_up_conf, d_lat_conf, B, H, W, d_scales, d_prior_focal, d_prior_gravity,
                             d_prior_dist, prior_dist_cols, d_cam_out, d_grav_out, d_info_out, nullptr, stream);
}

int gclm_system(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                const float* d_lat_conf, int B, int H, int W, const float* d_cam, const float* d_grav,
                int as_rpf, float* d_cost, float* d_grad, float* d_hess, void* stream) {
    if (!h) return -1;
    if (int rc = check_shapes(h, d_lat, B, H, W)) return rc;
    if (!d_cam || !d_grav || !d_cost || !d_grad || !d_hess) return fail(h, -3, "gclm_system: null pointer");
    h->sh.active = false;       // (as run_solve: also the empty call ends a split session)
    if (B == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(h->device);
    GCLM_HIP(h, guard.status);
    SolveCtx& c = h->ctx;
    c.n_groups = 0; c.group_size = 1; c.group_of_frame = nullptr; c.iso_final = 0;
    Plan p;      // one sweep: no plane of sin(latitude), handed or kept
    if (int rc = make_plan(h, p, Fields{d_up, d_lat, d_up_conf, d_lat_conf}, B, H, W, nullptr, 1)) return rc;
    GCLM_HIP(h, launch_pblock_from_params(c, d_cam, d_grav, as_rpf, c.pb_final, s));
    GCLM_HIP(h, launch_sweep(h->cfg.camera_model, p.next_sweep(h, c.pb_final, !as_rpf, 0), s));
    GCLM_HIP(h, launch_system_out(c, d_cost, d_grad, d_hess, s));
    return 0;
}

int gclm_shared_begin_ex(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                         const float* d_lat_conf, int B_local, int H, int W, float* d_cam_io,
                         float* d_grav_io, const int32_t* d_group_of_frame, int num_groups, const float* d_sin_lat,
                         void* stream) {
    if (!h) return -1;
    if (!h->cfg.shared_intrinsics) return fail(h, -2, "gclm_shared_begin: handle is not configured for shared_intrinsics");
    if (h->cfg.early_stop) return fail(h, -2, "gclm_shared_begin: early_stop needs a global decision; run with early_stop=0");
    if (int rc = check_shapes(h, d_lat, B_local, H, W)) return rc;
    if (!d_cam_io || !d_grav_io || !d_group_of_frame || num_groups <= 0) return fail(h, -3, "gclm_shared_begin: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(h->device);
    GCLM_HIP(h, guard.status);
    SolveCtx& c = h->ctx;
    c.n_groups = num_groups; c.group_size = 1; c.group_of_frame = d_group_of_frame; c.iso_final = 0;
    if (int rc = make_plan(h, h->sh.plan, Fields{d_up, d_lat, d_up_conf, d_lat_conf}, B_local, H, W, d_sin_lat, h->cfg.num_steps + 1,
                           false))
        return rc;
    h->sh.cam_io = d_cam_io; h->sh.grav_io = d_grav_io;
    h->sh.active = true;
    InitArgs ia{};
    ia.cam = d_cam_io;
    ia.grav = d_grav_io;
    GCLM_HIP(h, launch_init(c, ia, s));
    return 0;
}

int gclm_shared_begin(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                      const float* d_lat_conf, int B_local, int H, int W, float* d_cam_io,
                      float* d_grav_io, const int32_t* d_group_of_frame, int num_groups, void* stream) {
    return gclm_shared_begin_ex(h, d_up, d_lat, d_up_conf, d_lat_conf, B_local, H, W, d_cam_io, d_grav_io, d_group_of_frame,
                                num_groups, nullptr, stream);
}

int gclm_shared_reduce(gclm_handle* h, int step, float* d_partials, void* stream) {
    if (!h) return -1;
    if (!h->sh.active) return fail(h, -4, "gclm_shared_reduce: no active session (call gclm_shared_begin)");
    if (!d_partials || step < 0 || step >= h->cfg.num_steps) return fail(h, -3, "gclm_shared_reduce: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(h->device);
    GCLM_HIP(h, guard.status);
    SolveCtx& c = h->ctx;
    if (c.B > 0) {
        if (int rc = timed_sweep(h, h->sh.plan.next_sweep(h, c.pb[step & 1], true, 0), s)) return rc;
    }
    GCLM_HIP(h, launch_shared_reduce(c, step, d_partials, s));
    return 0;
}

int gclm_shared_apply(gclm_handle* h, int step, const float* d_partials, void* stream) {
    if (!h) return -1;
    if (!h->sh.active) return fail(h, -4, "gclm_shared_apply: no active session");
    if (!d_partials || step < 0 || step >= h->cfg.num_steps) return fail(h, -3, "gclm_shared_apply: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(h->device);
    GCLM_HIP(h, guard.status);
    if (h->ctx.B > 0) GCLM_HIP(h, launch_shared_apply(h->ctx, step, d_partials, s));
    return 0;
}

int gclm_shared_finish(gclm_handle* h, float* d_info_out, void* stream) {
    if (!h) return -1;
    if (!h->sh.active) return fail(h, -4, "gclm_shared_finish: no active session");
    if (!d_info_out) return fail(h, -3, "gclm_shared_finish: null info pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(h->device);
    GCLM_HIP(h, guard.status);
    SolveCtx& c = h->ctx;
    h->sh.active = false;
    if (c.B == 0) return 0;
    GCLM_HIP(h, launch_prep_final(c, s));
    if (int rc = timed_sweep(h, h->sh.plan.next_sweep(h, c.pb_final, false, 0), s)) return rc;
    GCLM_HIP(h, launch_finalize(c, h->sh.cam_io, h->sh.grav_io, d_info_out, s));
    return 0;
}

}  // extern "C"
