/*
 * gclm.h -- C ABI of libgeocalib_hip.so: GeoCalib's batched Levenberg-Marquardt calibration
 * (perspective-field residuals, analytic Jacobians, J^T W J / J^T W r reductions, damped solve,
 * manifold update) as hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference (cvg/GeoCalib) has no native/FFI boundary: its seam is the Python attribute
 * `GeoCalib.optimizer` (geocalib/geocalib.py:106,119), an `LMOptimizer` (geocalib/lm_optimizer.py:141).
 * Every entry point below states which reference function(s) it replaces.  All pointers named
 * `d_*` are DEVICE pointers owned by the caller (torch-ROCm tensors); `stream` is a hipStream_t
 * passed as void*.  Calls are asynchronous on `stream` and never synchronise the device -- with ONE exception: a
 * handle's workspace is allocated by the first solve and GROWN by the first solve of a larger shape than any before
 * (batch size, chunks per image, groups; the sin(latitude) scratch plane, an allocation of its own -- see
 * gclm_set_slat_plane): that call runs hipFree + hipMalloc, which synchronises the device once.  Every later call of that
 * shape or a smaller one finds the workspace in place: no allocation and no synchronisation after warm-up
 * (gclm_workspace_bytes reports its size, gclm_release_workspace gives it back).
 * Return value: 0 = ok, negative = error (message via gclm_last_error).  No C++ exception crosses
 * this boundary.  A handle is not thread-safe and owns the whole solve workspace: one handle per (device, stream).
 * Every entry point runs on the handle's device and restores the caller's current HIP device before it returns.
 * Numerical failure (non positive-definite system, or a NaN / inf step) is NOT an error: the image takes a zero
 * step and counts it in GCLM_INFO_STEP_FAILURES, like lm_optimizer.py:129-133 (there batch-global, here per image /
 * per shared group).
 * Degenerate inputs stay contained to their image and never hang (tests/test_gpu_parity.py::
 * test_bad_images_are_contained): an image with all-zero confidences keeps its initial estimate and reports a
 * non-finite covariance (the reference's torch.inverse raises on the singular Hessian); a NaN in a field makes every
 * step of THAT image fail (it keeps its initial estimate, its costs are NaN, the batch-global early stop then never
 * fires) and leaves the other images of the batch bit-identical to a clean run.
 * One call takes at most 65 535 images (grid.y); geocalib_amd.LMOptimizer slices larger batches.
 */
#ifndef GCLM_H
#define GCLM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: bumped whenever struct gclm_config or the export list changes (100 = round 1/2, 300 = round 3:
 * struct_size / abi_version / device moved into gclm_config, gclm_create lost its third argument, new entry points
 * gclm_set_sweep_iters, gclm_set_fused_steps, gclm_set_paced_launches, gclm_set_stop_comm, gclm_comm_all_reduce_sum_i32,
 * gclm_abi_config_size; 400 = round 4: gclm_comm_versions, gclm_merge_stop_at and gclm_upsample_fields_multi added, the NULL-handle error strings became thread-local, an
 * empty batch (B = 0, NULL fields) is accepted by gclm_solve / gclm_calibrate; 500 = round 5: gclm_set_slat_plane and gclm_plan_cut added;
 * 600 = round 6: gclm_set_slat_plane_limit, gclm_slat_plane_bytes, gclm_release_workspace and gclm_read_probe added, the
 * scratch plane became an optional allocation of its own, gclm_merge_stop_at skips empty parts; 610 = round 6: gclm_set_row_pairs
 * added -- radial / simple_divisional batches walk row pairs by default, results equal the one-row walk's to summation order;
 * additive within 610: gclm_pack_fields_ex, gclm_solve_ex, gclm_calibrate_ex and gclm_shared_begin_ex added -- the head
 * epilogue can write a plane of sin(latitude) that the solve reads, every existing entry point unchanged; gclm_undistort_image,
 * gclm_render_from_pano and gclm_perspective_fields added, also within 610; gclm_field_errors and
 * gclm_field_errors_workspace added, also within 610; gclm_hypothesis_scores and gclm_hypothesis_scores_workspace added, also
 * within 610; gclm_set_conf_pack, gclm_plan_conf_pack, gclm_conf_pack_bytes and gclm_conf_pack_fallbacks added, also within 610: large pinhole
 * batches keep their two confidence planes as one plane of 16-bit pairs, see gclm_set_conf_pack; gclm_rpf_hypotheses added, also
 * within 610: the three-pixel minimal solver whose rows gclm_hypothesis_scores ranks; gclm_reproject_image added, also within 610;
 * gclm_undistort_image_u8 and gclm_reproject_image_u8 added, also within 610: the two image calls for uint8 images;
 * gclm_draw_fields and gclm_draw_fields_u8 added, also within 610: the perspective fields drawn over an image;
 * gclm_pack_fields_bins added, also within 610: the head epilogue for classification heads;
 * gclm_param_opt, gclm_param_opt_cost, gclm_param_opt_step, gclm_param_opt_workspace and gclm_default_param_opt_config added, also
 * within 610: Adam on (roll, pitch, vfov) against perspective fields, the reference's third optimiser;
 * gclm_field_loss, gclm_field_loss_grad and gclm_field_loss_workspace added, also within 610: the decoders' training losses
 * against a calibration and their gradients with respect to the predicted fields;
 * gclm_solve_recorded, gclm_calibrate_recorded, gclm_lm_backward and gclm_lm_backward_workspace added, also within 610: the
 * solve with a step record, and the adjoint of its LM steps -- the gradients of the optimised camera and gravity with respect
 * to the fields and the confidences;
 * gclm_pack_fields_typed and gclm_pack_fields_backward added, also within 610: the head epilogue for float16 / bfloat16 raw
 * planes, and its backward -- the gradients of the fields and confidences taken back to the raw head outputs in one pass;
 * gclm_field_loss_param_grad, gclm_perspective_fields_backward and gclm_field_param_grad_workspace added, also within 610: the
 * gradients of the field losses, and of the rendered fields, with respect to the camera and the gravity;
 * gclm_calibrate_soft added, also within 610: gclm_calibrate_ex with a focal and a gravity prior given with their standard
 * deviations, as pseudo-observations of every LM step and of the uncertainty pass;
 * gclm_bin_loss, gclm_bin_loss_grad and gclm_bin_loss_workspace added, also within 610: the classification heads' training
 * loss -- per-pixel cross-entropy of the logits against the bins of a calibration's fields -- and its gradient to the logits).
 * gclm_create refuses a gclm_config whose first two fields do not
 * carry the library's own sizeof(gclm_config) and GCLM_VERSION, with a message naming both sides. */
#define GCLM_VERSION 610

/* camera_models of geocalib/camera.py:945-950 */
enum gclm_camera_model {
    GCLM_PINHOLE = 0,           /* camera.py:522 */
    GCLM_SIMPLE_RADIAL = 1,     /* camera.py:565 */
    GCLM_RADIAL = 2,            /* camera.py:663 */
    GCLM_SIMPLE_DIVISIONAL = 3  /* camera.py:789 */
};

#define GCLM_MAX_PARAMS 5     /* delta_g1, delta_g2, focal, k1, k2 */
#define GCLM_MAX_STEPS 256
#define GCLM_MAX_RECALL_THRESHOLDS 8     /* gclm_field_errors */
#ifndef GCLM_HYPOTHESIS_CHUNK
#define GCLM_HYPOTHESIS_CHUNK 16         /* gclm_hypothesis_scores: hypotheses scored per read of an image's planes */
#endif
#define GCLM_RPF_MAX_SAMPLES (1 << 24)   /* gclm_rpf_hypotheses: most samples per image of one call */
#define GCLM_RPF_DRAW_SALT 0x5250465F44524157ull   /* gclm_rpf_hypotheses: mixed into the seed of the in-kernel draw */
#define GCLM_CAM_STRIDE 8     /* {w,h,fx,fy,cx,cy,k1,k2}: BaseCamera._data, camera.py:25-41 */
#define GCLM_GRAV_STRIDE 3    /* unit gravity: Gravity._data, gravity.py:18-28 */

/* info_out row layout (floats) -- the `infos` dict of lm_optimizer.py:575,586-588,509-516,638-642 */
#define GCLM_INFO_STRIDE 48
enum gclm_info_slot {
    GCLM_INFO_STOP_AT = 0,
    GCLM_INFO_INITIAL_UP_COST = 1,
    GCLM_INFO_INITIAL_LAT_COST = 2,
    GCLM_INFO_INITIAL_COST = 3,
    GCLM_INFO_FINAL_UP_COST = 4,
    GCLM_INFO_FINAL_LAT_COST = 5,
    GCLM_INFO_FINAL_COST = 6,
    GCLM_INFO_ROLL_UNC = 7,
    GCLM_INFO_PITCH_UNC = 8,
    GCLM_INFO_GRAVITY_UNC = 9,
    GCLM_INFO_FOCAL_UNC = 10,
    GCLM_INFO_VFOV_UNC = 11,
    GCLM_INFO_NPARAMS = 12,
    GCLM_INFO_LAMBDA = 13,         /* after every update_lambda of the solve: one per comparison made, the one that fired an early stop included */
    GCLM_INFO_STEP_FAILURES = 14,  /* number of LM steps rejected: Cholesky failed or the step was NaN / inf (zero step) */
    GCLM_INFO_COV = 16             /* covariance, P x P row-major, up to 25 floats */
};

/*
 * Mirrors LMOptimizer.default_conf (lm_optimizer.py:144-162) plus what
 * setup_optimization_and_priors (lm_optimizer.py:189-246) derives from the priors.
 */
typedef struct gclm_config {
    int32_t struct_size;             /* sizeof(gclm_config) of the CALLER's header (set by gclm_default_config) */
    int32_t abi_version;             /* GCLM_VERSION of the CALLER's header (set by gclm_default_config) */
    int32_t device;                  /* HIP device ordinal the handle is bound to (LMOptimizer(...).to(device)) */
    int32_t camera_model;            /* enum gclm_camera_model */
    int32_t shared_intrinsics;       /* lm_optimizer.py:147; groups of `group_size` frames */
    int32_t group_size;              /* frames per shared-intrinsics group; 0 = whole batch (reference) */
    int32_t num_steps;               /* :149 */
    float lambda0;                   /* :150 */
    int32_t fix_lambda;              /* :151 */
    int32_t early_stop;              /* :152 (batch-global, :90-92,:619-625) */
    float atol, rtol;                /* :153-154; the test |new - prev| <= atol + |rtol * prev| is evaluated in float32, as
                                        torch.allclose does for float32 costs (the scalar tolerances do not promote) */
    int32_t use_spherical_manifold;  /* :155 */
    int32_t use_log_focal;           /* :156 */
    float up_loss_fn_scale;          /* :158 */
    float lat_loss_fn_scale;         /* :159 */
    int32_t estimate_gravity;        /* :204-207 (0 when prior_gravity is given) */
    int32_t estimate_focal;          /* :209-212 */
    int32_t estimate_dist;           /* :214-221 */
    int32_t compute_uncertainty;     /* eval mode: estimate_uncertainty (:635-636) */
    int32_t heuristic_init;          /* gclm_calibrate only: siclib's get_heuristic_estimation instead of the trivial
                                        estimate (siclib/models/optimization/utils.py:27-82; needs the up field) */
} gclm_config;

typedef struct gclm_handle gclm_handle;

/* Library / ABI version (GCLM_VERSION of the build) and the sizeof(gclm_config) the library was built with. */
int gclm_version(void);
int gclm_abi_config_size(void);

/* Fill `cfg` with LMOptimizer.default_conf (lm_optimizer.py:144-162), everything estimated, eval mode, device 0,
 * and the library's own struct_size / abi_version.  A caller compiled against another header therefore passes the
 * check of gclm_create only if its struct really has the library's layout: compare gclm_abi_config_size() with the
 * caller's sizeof(gclm_config) (and gclm_version() with GCLM_VERSION) BEFORE calling this with a smaller struct. */
int gclm_default_config(gclm_config* cfg);

/* LMOptimizer.__init__ (lm_optimizer.py:164-171): validate the configuration, bind to cfg->device.  Signature as
 * SURVEY.md section 8(b).  Fails (-5, message via gclm_last_error(NULL)) when cfg->struct_size / cfg->abi_version
 * are not the library's: a stale caller is told so instead of handing over a too-small struct. */
int gclm_create(gclm_handle** out, const gclm_config* cfg);

/* Re-configure (set_camera_model :173, .shared_intrinsics, priors) without dropping the workspace.  The device of a
 * handle cannot change.  A call after gclm_configure returns what the same call returns on a handle freshly created with
 * that configuration and the same knobs, bit for bit, whatever the handle did before (tests/test_handle_reuse.py); a split
 * session that was open is over. */
int gclm_configure(gclm_handle* h, const gclm_config* cfg);

int gclm_destroy(gclm_handle* h);

/* Message of the last failing call on this handle; h == NULL: of the last failing gclm_create of the CALLING THREAD
 * (thread-local storage: two threads creating handles do not see each other's message). */
const char* gclm_last_error(const gclm_handle* h);

/* Bytes of device scratch the handle holds (grows on demand in gclm_solve, never per call after warm-up): the core
 * workspace (per-image states, parameter blocks, partial records: ~3 KB per image) plus the sin(latitude) scratch plane
 * and the packed confidence plane where one is held (gclm_slat_plane_bytes, gclm_conf_pack_bytes: H x W x 4 bytes per image each). */
size_t gclm_workspace_bytes(const gclm_handle* h);
size_t gclm_slat_plane_bytes(const gclm_handle* h);
/* Give the handle's device memory back (hipFree: waits for the device, so nothing of the handle is in flight after).  The
 * handle stays valid; its next solve allocates again.  For serving loops that have seen a rare huge batch. */
int gclm_release_workspace(gclm_handle* h);

/*
 * LMOptimizer.optimize (lm_optimizer.py:551-644) for B images of H x W pixels: all LM steps,
 * the final costs and (compute_uncertainty) estimate_uncertainty (:463-516).
 *   d_up        (B,2,H,W) float32 up field, or NULL          (data["up_field"])
 *   d_lat       (B,1,H,W) float32 latitude in radians        (data["latitude_field"], required like :31)
 *   d_up_conf   (B,H,W)   float32 or NULL                    (data["up_confidence"])
 *   d_lat_conf  (B,H,W)   float32 or NULL                    (data["latitude_confidence"])
 *   d_cam_io    (B,8)     in: initial camera (get_trivial_estimation :20-58), out: optimised camera
 *   d_grav_io   (B,3)     in: initial unit gravity, out: optimised gravity
 *   d_info_out  (B,GCLM_INFO_STRIDE) float32, see enum gclm_info_slot
 */
int gclm_solve(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
               const float* d_lat_conf, int B, int H, int W, float* d_cam_io, float* d_grav_io,
               float* d_info_out, void* stream);

/*
 * LMOptimizer.forward (lm_optimizer.py:646-664): get_trivial_estimation (:20-58; roll = pitch = 0,
 * f = 0.7 max(h, w) through the vfov round trip, principal point at the centre, priors substituted) evaluated
 * on the device, then gclm_solve.  No host-side tensor op is needed before the call.
 *   d_scales         (2,)   or NULL   data["scales"]:  fx = f * scales[0] / scales[1]   (camera.py:89-90)
 *   d_prior_focal    (B,)   or NULL   data["prior_focal"]   (requires cfg.estimate_focal == 0)
 *   d_prior_gravity  (B,3)  or NULL   data["prior_gravity"] (requires cfg.estimate_gravity == 0)
 *   d_prior_dist     (B,prior_dist_cols) or NULL   data["prior_dist"]
 *   d_cam_out (B,8), d_grav_out (B,3), d_info_out (B,GCLM_INFO_STRIDE): outputs
 */
int gclm_calibrate(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                   const float* d_lat_conf, int B, int H, int W, const float* d_scales,
                   const float* d_prior_focal, const float* d_prior_gravity, const float* d_prior_dist,
                   int prior_dist_cols, float* d_cam_out, float* d_grav_out, float* d_info_out, void* stream);

/*
 * gclm_solve / gclm_calibrate with one more argument, d_sin_lat: (B,1,H,W) float32 holding sin(latitude_field), laid out
 * like d_lat -- the sixth plane of gclm_pack_fields_ex, or the caller's own sin of d_lat -- or NULL (= gclm_solve /
 * gclm_calibrate exactly; those two are these with NULL).  d_lat stays required: the plane is an optional accelerator.
 * Each of the num_steps + 1 sweeps of a solve takes sin(latitude_field) again (lm_optimizer.py:262,270); with the plane
 * handed, the sweeps that can read it do so IN PLACE OF d_lat, from the first sweep of the solve to the final uncertainty
 * sweep, and the library holds no scratch plane for the solve (see gclm_set_slat_plane: none is allocated; one the handle
 * already holds is kept, unused).  Where the plane is read:
 *   - the five-plane (both confidences) 16-byte-aligned sweeps of simple_radial, radial and simple_divisional, on the
 *     one-row walk and on row pairs (gclm_set_row_pairs);
 *   - the same sweeps in a shared-intrinsics session (gclm_shared_begin_ex ... gclm_shared_finish);
 *   - the five-plane one-launch-per-step path (gclm_set_fused_steps; single images), for all four camera models.
 * Everywhere else the plane is ignored and d_lat is read as by gclm_solve: pinhole's batch sweeps (memory-bound), the scalar
 * path (W % 4 != 0 or a field plane not 16-byte aligned), four-plane and latitude-only sweeps, and a d_sin_lat that is not
 * 16-byte aligned while the other planes are.  The initial estimate (cfg.heuristic_init) always reads d_lat.
 * The result of a solve that reads the plane is that of a solve from d_lat bit for bit when the plane holds the library's
 * own sin of d_lat (gclm_pack_fields_ex); a caller's own sin (e.g. torch.sin) may differ in the last bit per pixel.
 */
int gclm_solve_ex(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                  const float* d_lat_conf, int B, int H, int W, float* d_cam_io, float* d_grav_io,
                  float* d_info_out, const float* d_sin_lat, void* stream);
int gclm_calibrate_ex(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                      const float* d_lat_conf, int B, int H, int W, const float* d_scales,
                      const float* d_prior_focal, const float* d_prior_gravity, const float* d_prior_dist,
                      int prior_dist_cols, float* d_cam_out, float* d_grav_out, float* d_info_out,
                      const float* d_sin_lat, void* stream);

/*
 * gclm_solve / gclm_calibrate with a step record: d_record is NULL -- the call is gclm_solve_ex / gclm_calibrate_ex with a
 * NULL d_sin_lat -- or (B, num_steps, GCLM_LM_RECORD_STRIDE) float32 on the device, which the call zeroes and the per-image
 * update of every LM step that runs fills, one row per step:
 *   [GCLM_LM_RECORD_CAMERA .. +8)   the camera row the step started from (w h fx fy cx cy k1 k2)
 *   [GCLM_LM_RECORD_GRAVITY .. +3)  ... and its gravity
 *   [GCLM_LM_RECORD_LAMBDA]         the damping the step used (the rule of lm_optimizer.py:95-106 applied)
 *   [GCLM_LM_RECORD_DELTA .. +5)    the solution of the damped normal equations over the full columns (d1, d2, focal, k1, k2):
 *                                   zero in fixed columns, all zero after a failed Cholesky
 *   [GCLM_LM_RECORD_FAILED]         1 if the Cholesky failed (the step is the zero step), else 0
 *   [GCLM_LM_RECORD_EXECUTED]       1
 *   [GCLM_LM_RECORD_SYSTEM .. +24)  the reduced accumulator record of the step's sweep: sum cost up, sum cost latitude, J^T W r
 *                                   over the PM = 4 (radial: 5) full columns, the upper triangle of J^T W J row-major
 * With early_stop the update at which the stop fires (step stop_at) still leaves its row: the state it computed is discarded, so
 * the rows of a solve are [0, stop_at) then; rows after it stay zero.  The record holds values the update computes anyway:
 * results equal those of the call without a record bit for bit (a call that would take one launch per LM step takes the
 * two-launch sequence, its twin bit for bit).  Per-image solves only: -3 with shared_intrinsics.
 */
#define GCLM_LM_RECORD_STRIDE 48
#define GCLM_LM_RECORD_CAMERA 0
#define GCLM_LM_RECORD_GRAVITY 8
#define GCLM_LM_RECORD_LAMBDA 11
#define GCLM_LM_RECORD_DELTA 12
#define GCLM_LM_RECORD_FAILED 17
#define GCLM_LM_RECORD_EXECUTED 18
#define GCLM_LM_RECORD_SYSTEM 24
int gclm_solve_recorded(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                        const float* d_lat_conf, int B, int H, int W, float* d_cam_io, float* d_grav_io,
                        float* d_info_out, float* d_record, void* stream);
int gclm_calibrate_recorded(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                            const float* d_lat_conf, int B, int H, int W, const float* d_scales,
                            const float* d_prior_focal, const float* d_prior_gravity, const float* d_prior_dist,
                            int prior_dist_cols, float* d_cam_out, float* d_grav_out, float* d_info_out,
                            float* d_record, void* stream);

/*
 * gclm_calibrate_ex with SOFT priors: a prior given together with its standard deviation is not frozen but enters every LM
 * step, the compared cost and the uncertainty pass as one more observation.  An extension (the reference's priors are all
 * or nothing), in the reference's conventions: cost = sum rho / N, H = sum w J^T J, G = sum w J^T r with r = target - model,
 * step (H + damp) delta = G, Cov = H^-1.
 *   d_prior_focal_sigma    (B,) or NULL  standard deviation of d_prior_focal, in pixels of fy; needs d_prior_focal and
 *                                        cfg.estimate_focal == 1 (the column stays free)
 *   d_prior_gravity_sigma  (B,) or NULL  isotropic standard deviation of d_prior_gravity, in radians; needs d_prior_gravity
 *                                        and cfg.estimate_gravity == 1
 *   d_prior_cost_out       (B,2) or NULL the priors' cost / N at the initial and at the final state
 * Both in the units of the solve's own covariance (GCLM_INFO_COV: unit residual noise), not of a calibrated physical noise.
 * A prior without its sigma is the hard prior of gclm_calibrate (its estimate_* flag 0); the two may be mixed.  Either prior
 * seeds the initial estimate exactly as the hard one does.  At state (g, fy), per LM step, added to the image's reduced system:
 *   focal    on the log-focal column: w = (f0 / sigma_f)^2, r = log f0 - log fy;  G[2] += w r, H[2][2] += w, cost += w r^2
 *   gravity  g0 = normalize(prior), w = 1 / sigma_g^2, r = g0 - g, T the 3x2 tangent basis of the gravity columns;
 *            G[0:2] += w T^T r, H[0:2,0:2] += w T^T T, cost += w |r|^2
 * The cost that the damping rule and the early stop compare is up + latitude + prior / N, each term at the same state;
 * GCLM_INFO_INITIAL_COST and GCLM_INFO_FINAL_COST are those sums (final: the float32 sum (up + latitude) + prior / N of the
 * values reported), the up and latitude slots stay the data's.  The uncertainty pass adds T^T T / sigma_g^2 (T: the roll-pitch
 * tangent) and 1 / sigma_f^2 on the plain-focal diagonal before the inverse: the covariance is the posterior's.
 * A sigma that is not finite and > 0 (or a prior focal that is not, or a prior gravity that does not normalise) leaves its term
 * out for that image and counts one into GCLM_INFO_STEP_FAILURES per LM step.  A sigma so large that its weight underflows
 * adds exact zeros: the result is the two-launch solve's without the prior, bit for bit.
 * The LM step of such a call is always two launches (sweep, per-image update): the priors are added by the update kernel.
 * With both sigma pointers NULL the call is gclm_calibrate_ex exactly (d_prior_cost_out is not written).  Otherwise it returns
 * -3, before the handle is looked at and before any HIP call, for a sigma without its prior, B <= 0 or beyond 65535, H or W
 * <= 0, a NULL latitude or output, prior_dist_cols outside 1 .. 2, a pointer that is not 4-byte aligned, or an output that
 * overlaps another range of the call; then -1 for a NULL handle, -3 for shared_intrinsics or use_spherical_manifold /
 * use_log_focal off, and -2 where an estimate_* flag disagrees with the priors (a soft prior's flag is 1).
 */
int gclm_calibrate_soft(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                        const float* d_lat_conf, int B, int H, int W, const float* d_scales,
                        const float* d_prior_focal, const float* d_prior_gravity, const float* d_prior_dist,
                        int prior_dist_cols, const float* d_prior_focal_sigma, const float* d_prior_gravity_sigma,
                        float* d_cam_out, float* d_grav_out, float* d_info_out, float* d_prior_cost_out,
                        const float* d_sin_lat, void* stream);

/*
 * gclm_lm_backward: the adjoint of the LM steps of a recorded solve (no handle).  Given the gradients of a scalar with respect
 * to the solve's outputs, d_grad_cam (B, 8) (columns fx, fy, k1, k2 are read; the size and the principal point are constants
 * of the solve) and d_grad_grav (B, 3), it writes the gradients with respect to the inputs whose plane is given: d_grad_up
 * (B, 2, H, W), d_grad_lat (B, 1, H, W), d_grad_up_conf and d_grad_lat_conf (B, H, W).  A NULL plane is neither computed nor
 * written; a plane whose input is absent must be NULL.  No gradient flows through the damping (it depends on the costs
 * through a comparison), the initial estimate or the priors.
 *
 * One step at state theta with the step delta = A^-1 G, A = H + diag(clamp(lambda H_jj, 1e-6)), theta+ = theta [+] delta
 * (lm_optimizer.py:109-137, 518-549).  With the incoming adjoint of theta+: a per-image kernel takes the adjoint of [+]
 * (Householder plus on the sphere, exp(log f + delta_f) with fx following fy, the clamped distortion) in forward mode,
 * solves v = A^-1 delta-bar from the recorded system and forms the mask m_j = [lambda H_jj > 1e-6]; a pass over the planes
 * evaluates, per pixel in registers,
 *   phi = w [ (J v) . r - (J v) . (J delta) - lambda sum_j m_j v_j delta_j |J_j|^2 ]        (per field; v, delta, m frozen)
 * with its derivatives with respect to the pixel's inputs (added into the gradient planes: the first processed step stores,
 * later ones accumulate) and to theta (one float64 record per tile, summed per image by a finish kernel, no atomics).  J is
 * the forward-mode derivative of the fields at theta [+] delta', delta' = 0, and its derivative with respect to theta a second
 * forward-mode level over the same scalar-templated field formulas.  Steps run from the last executed one down to step 0:
 * num_steps of them, or, with early_stop != 0, the first stop_at that d_info (the solve's info rows) names.
 *
 * camera_model: GCLM_PINHOLE or GCLM_SIMPLE_RADIAL (-3 otherwise); spherical manifold and log focal length.  up_scale /
 * lat_scale: the Huber scales of the solve (2^20 for the squared loss).  estimate_*: the solve's free-parameter flags.
 * d_workspace: at least gclm_lm_backward_workspace(B, H, W) bytes (0: sizes out of range), 8-byte aligned.  Returns -3 for
 * NULL or misaligned pointers, overlapping outputs, num_steps outside 1..GCLM_MAX_STEPS and sizes out of range.
 */
size_t gclm_lm_backward_workspace(int B, int H, int W);
int gclm_lm_backward(int camera_model, const float* d_up, const float* d_lat, const float* d_up_conf, const float* d_lat_conf,
                     int B, int H, int W, const float* d_record, int num_steps, int early_stop, const float* d_info,
                     float up_scale, float lat_scale, int estimate_gravity, int estimate_focal, int estimate_dist,
                     const float* d_grad_cam, const float* d_grad_grav, float* d_grad_up, float* d_grad_lat,
                     float* d_grad_up_conf, float* d_grad_lat_conf, void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * One fused sweep at fixed parameters: calculate_residuals + calculate_costs + setup_system
 * (lm_optimizer.py:248-315,387-461).  as_rpf selects the (roll, pitch, focal) parametrisation used
 * by estimate_uncertainty (:481-483).  Outputs, per image: d_cost (B,2) mean up / latitude Huber cost,
 * d_grad (B,5) and d_hess (B,5,5) over the full column set [d1,d2,f,k1,k2] (unused columns zero).
 */
int gclm_system(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                const float* d_lat_conf, int B, int H, int W, const float* d_cam, const float* d_grav,
                int as_rpf, float* d_cost, float* d_grad, float* d_hess, void* stream);

/*
 * Shared-intrinsics solve with a group's frames split over several devices (BASELINE config 5).
 * The caller drives the LM loop: per step, gclm_shared_reduce leaves, for each of the G groups,
 * the local Schur partials [sum E^T D^-1 E (3 x 3) | sum E^T D^-1 g (3) | sum H_ii (3 x 3) | sum g_i (3) | #frames]
 * over its ni <= 3 shared intrinsics (unused entries zero)
 * in d_partials (G x GCLM_SHARED_PARTIAL_STRIDE floats); the caller all-reduces (sum) that buffer over the
 * ranks holding frames of the same groups (RCCL), then gclm_shared_apply solves and updates its frames.
 * Together they replace the dense arrow-head Cholesky of lm_optimizer.py:350-383,:597-603.
 */
#define GCLM_SHARED_PARTIAL_STRIDE 32
int gclm_shared_begin(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                      const float* d_lat_conf, int B_local, int H, int W, float* d_cam_io,
                      float* d_grav_io, const int32_t* d_group_of_frame /* (B_local), non-decreasing */,
                      int num_groups, void* stream);
/* gclm_shared_begin with a plane of sin(latitude_field) (NULL = gclm_shared_begin), read by the session's sweeps under the
 * rule of gclm_solve_ex.  Like the field pointers, d_sin_lat must stay valid until gclm_shared_finish. */
int gclm_shared_begin_ex(gclm_handle* h, const float* d_up, const float* d_lat, const float* d_up_conf,
                         const float* d_lat_conf, int B_local, int H, int W, float* d_cam_io,
                         float* d_grav_io, const int32_t* d_group_of_frame /* (B_local), non-decreasing */,
                         int num_groups, const float* d_sin_lat, void* stream);
int gclm_shared_reduce(gclm_handle* h, int step, float* d_partials, void* stream);
int gclm_shared_apply(gclm_handle* h, int step, const float* d_partials, void* stream);
int gclm_shared_finish(gclm_handle* h, float* d_info_out, void* stream);

/*
 * The step BEFORE the path: the CNN head epilogues UpDecoder / LatitudeDecoder (geocalib/geocalib.py:57,73-75)
 * fused into one pass that writes the planes gclm_calibrate reads:
 *   up = normalize(up_raw, dim=1)  (eps 1e-12),   latitude = asin(clamp(tanh(lat_raw), +-(1 - 1e-5))),
 *   up_conf = sigmoid(up_logconf),                lat_conf = sigmoid(lat_logconf)     (NULL: skipped)
 * Shapes: up_raw / up (B,2,H,W); lat_raw / lat (B,1,H,W); log-confidences / confidences (B,H,W).  In-place
 * operation (output pointer == input pointer) is allowed.
 */
int gclm_pack_fields(const float* d_up_raw, const float* d_up_logconf, const float* d_lat_raw,
                     const float* d_lat_logconf, int B, int H, int W, float* d_up, float* d_up_conf, float* d_lat,
                     float* d_lat_conf, void* stream);
/* The same pass (the five planes bit-identical to gclm_pack_fields', which is this with NULL), writing, when d_sin_lat
 * (B,1,H,W) is not NULL, a sixth plane in the same launch: sin of the latitude it has just written, by the polynomial the
 * sweeps use -- the plane gclm_solve_ex / gclm_calibrate_ex / gclm_shared_begin_ex read in place of d_lat, with the results
 * of a solve from d_lat bit for bit.  d_sin_lat must not overlap any other plane of the call (-3).  A d_sin_lat that is not
 * 16-byte aligned sends the pass to its scalar path (as any other unaligned plane does). */
int gclm_pack_fields_ex(const float* d_up_raw, const float* d_up_logconf, const float* d_lat_raw,
                        const float* d_lat_logconf, int B, int H, int W, float* d_up, float* d_up_conf, float* d_lat,
                        float* d_lat_conf, float* d_sin_lat /* (B,1,H,W) or NULL */, void* stream);

/*
 * gclm_pack_fields_ex for raw planes of raw_dtype (enum gclm_logit_dtype below: float32, float16, bfloat16; all raw planes of
 * a call share it); the outputs are float32.  Each element widens exactly and the arithmetic is gclm_pack_fields_ex's, in
 * float32: GCLM_LOGITS_F32 gives its bits (and is that call), a 16-bit type the bits of gclm_pack_fields_ex on the widened
 * planes.  In-place operation stays legal for float32 only.  For the 16-bit types, -3: a NULL d_up_raw, d_lat_raw, d_up or
 * d_lat; B < 0, H or W <= 0; a log-confidence without its output; a raw plane off a 2-byte, an output off a 4-byte boundary;
 * an output that overlaps any other plane of the call.  -3 for an unknown raw_dtype.  B = 0 succeeds and launches nothing.
 * Where H * W is a multiple of 8 and every plane is 16-byte aligned a lane reads eight pixels with one 16-byte load per
 * plane; any other call takes one pixel per lane, same results.
 */
int gclm_pack_fields_typed(int raw_dtype, const void* d_up_raw, const void* d_up_logconf, const void* d_lat_raw,
                           const void* d_lat_logconf, int B, int H, int W, float* d_up, float* d_up_conf, float* d_lat,
                           float* d_lat_conf, float* d_sin_lat /* (B,1,H,W) or NULL */, void* stream);
/*
 * The BACKWARD of that pass: the float32 gradients d_g_* of its four outputs (d_g_up (B,2,H,W), the others (B,H,W)) taken
 * back to the raw planes, d_d_*, written in raw_dtype (rounded to nearest even from the float32 value).  One pass; it reads
 * the raw planes again and recomputes in float32 what it needs -- no forward output is read, none has to be kept.  There is
 * no gradient for the sin(latitude) plane.  Per pixel:
 *   up          n = |r|;  n >= 1e-12: d_r = (g - u (u . g)) / n with u = r / n, evaluated as u' (u' . g) / n, u' = (-u.y, u.x)
 *               (the same vector in two dimensions, without the cancellation);  n < 1e-12: d_r = g / 1e-12
 *   latitude    d_x = g sech(x) = g 2 e / (1 + e^2), e = exp(-|x|), where tanhf(x) lies within [-1 + 1e-5, 1 - 1e-5], bounds
 *               included; exactly 0 outside -- the forward's own comparison, so both agree on every pixel
 *   confidence  d_x = g s (1 - s) = g e / (1 + e)^2, e = exp(-|x|): finite for every finite x
 * A NaN raw value gives NaN gradients in its own group (up, latitude, either confidence) only.
 * Any d_g_* may be NULL (that output got no gradient) and any d_d_* may be NULL (that gradient is not wanted); a d_d_* that is
 * given needs its d_g_* and its raw plane, and a group whose d_d_* is NULL is not read.
 * -3: an unknown raw_dtype; B < 0, H or W <= 0; no d_d_* at all; a d_d_* without its d_g_* or its raw plane; a pointer off its
 * element's alignment (raw_dtype's for raws and d_d_*, 4 bytes for d_g_*); a d_d_* that overlaps any other plane of the call.
 * B = 0 succeeds and launches nothing.  16-byte accesses (four floats; eight 16-bit elements against two float4 of gradient)
 * where H * W is a multiple of the pixels per lane and every plane read or written is 16-byte aligned; else one pixel per lane.
 */
int gclm_pack_fields_backward(int raw_dtype, const void* d_up_raw, const void* d_up_logconf, const void* d_lat_raw,
                              const void* d_lat_logconf, int B, int H, int W, const float* d_g_up, const float* d_g_up_conf,
                              const float* d_g_lat, const float* d_g_lat_conf, void* d_d_up_raw, void* d_d_up_logconf,
                              void* d_d_lat_raw, void* d_d_lat_logconf, void* stream);

/*
 * The same step for CLASSIFICATION heads (siclib's UpDecoder / LatitudeDecoder with loss_type == "classification", the format
 * of the original PerspectiveFields weights; siclib/models/utils/perspective_encoding.py): the up head emits up_bins logits per
 * pixel (73: one per 5 degrees and an "invalid" class), the latitude head lat_bins (180: one per degree), and the fields are
 * the decodes of the per-pixel argmax.  One pass reads d_up_logits (B,up_bins,H,W) and d_lat_logits (B,lat_bins,H,W) --
 * contiguous, both of the type logit_dtype -- once and writes the planes gclm_calibrate reads:
 *   u = argmax_k up_logits[b,k,y,x]      up[b,0,y,x] = up_table[u][0]     up[b,1,y,x] = up_table[u][1]
 *   l = argmax_k lat_logits[b,k,y,x]     lat[b,0,y,x] = lat_table[l]
 *   up_conf = sigmoid(up_logconf), lat_conf = sigmoid(lat_logconf)   (NULL: skipped; the floats gclm_pack_fields writes)
 *   sin_lat = sin(lat) by the sweeps' polynomial                      (NULL: skipped; the plane of gclm_pack_fields_ex)
 * argmax is torch.argmax's: the FIRST index of the greatest value; a NaN counts as greater than everything and the first NaN
 * wins; a pixel whose logits are all -inf gives 0.  16-bit logits are compared as the floats they widen to.
 * The two tables are the caller's, float32 in device memory, and hold the decode of every bin; the kernel only gathers from
 * them, so its output is the table's bits.  The reference's decodes, every operation in float32 in the order written (the
 * constants 360.0 / (up_bins - 1), s = 180.0 / lat_bins, s / 2 and pi formed in double and rounded to float32 once):
 *   up_table[k]  = (cos(a), sin(a)),  a = (k * (360 / (up_bins - 1)) - 180) / 180 * pi,   k < up_bins - 1
 *   up_table[up_bins - 1] = (0, 0)                                      (the invalid class)
 *   lat_table[k] = (e_k + s / 2) / 180 * pi,   e_k = the float32 nearest to -90 + k * s (that sum in double)
 * (geocalib_amd.perspective_encoding.up_bin_table / latitude_bin_table build them with torch on the CPU: the reference's
 * floats.)  Every lat_table entry must lie within +-pi/2, as bin centres do: sin_lat is evaluated without a range fold.
 * -3: a NULL logit tensor, table, d_up or d_lat; up_bins < 2, lat_bins < 1 or either above GCLM_MAX_BINS; an unknown
 * logit_dtype; H or W <= 0, B < 0; a log-confidence without its output; a pointer off its element's alignment; an output that
 * overlaps a logit tensor, a table or another output; d_sin_lat overlapping anything.  A log-confidence may be converted in
 * place (output pointer == input pointer; any other overlap of the two is refused).  B = 0 succeeds and launches nothing.
 * Where H * W is a multiple of the pixels per lane (4 for float32, 8 for the 16-bit types) and every plane is 16-byte
 * aligned, each channel is read with one 16-byte load per lane; any other call takes one pixel per lane, same results.
 */
enum gclm_logit_dtype { GCLM_LOGITS_F32 = 0, GCLM_LOGITS_F16 = 1, GCLM_LOGITS_BF16 = 2 };
#define GCLM_MAX_BINS 2048
int gclm_pack_fields_bins(const void* d_up_logits, int up_bins, const void* d_lat_logits, int lat_bins, int logit_dtype,
                          const float* d_up_table /* (up_bins,2) */, const float* d_lat_table /* (lat_bins) */,
                          const float* d_up_logconf, const float* d_lat_logconf, int B, int H, int W, float* d_up,
                          float* d_up_conf, float* d_lat, float* d_lat_conf, float* d_sin_lat /* (B,1,H,W) or NULL */,
                          void* stream);

/*
 * The step AFTER the path: GeoCalib._post_process (geocalib/extractor.py:51-69) resizes the fields and confidences
 * back to the input resolution with F.interpolate(mode="bilinear", align_corners=False).  `planes` = number of
 * contiguous (h, w) planes in d_src (e.g. B*2 for the up field); d_dst holds planes x (H, W).
 * The sources must be FINITE: the vector path reads a window of 4 or 5 consecutive source floats per lane and multiplies
 * the ones an output does not tap by an exact 0, so a NaN / Inf source pixel reaches up to four output pixels beyond the
 * ones F.interpolate would make non-finite (which itself turns a zero-weight non-finite tap into NaN).  The CNN-head
 * outputs this entry point exists for (unit up vectors, asin(tanh) latitudes, sigmoid confidences) are always finite.
 */
int gclm_upsample_fields(const float* d_src, int planes, int h, int w, int H, int W, float* d_dst, void* stream);
/* ... and the same for up to 8 tensors of (h, w) planes in ONE launch (the four tensors _post_process resizes: a
 * single-image calibrate() pays one launch instead of four). */
int gclm_upsample_fields_multi(const float* const* d_srcs, float* const* d_dsts, const int* planes, int n_tensors, int h, int w,
                               int H, int W, void* stream);

/*
 * BaseCamera.undistort_image (geocalib/camera.py:396-412) for a batch, in one pass: d_dst (B, C, H, W) is d_src
 * (B, C, Hin, Win) resampled at the distorted position of every output pixel, float32 NCHW.  d_cam is (cam_batch, 8)
 * {w, h, fx, fy, cx, cy, k1, k2} in device memory (read by the kernel; the w, h entries are not read: H, W are the output
 * size); cam_batch = 1 shares one camera over the batch, cam_batch = B gives each image its own.  For output pixel (x, y),
 * integer pixel centres, no half-pixel offset:
 *   u = (x - cx) / fx,  v = (y - cy) / fy,  r2 = u^2 + v^2,  s = the model's distort scale s(r2)
 *   ix = ((x - cx) s + cx) (Win - 1) / (W - 1),   iy = ((y - cy) s + cy) (Hin - 1) / (H - 1)
 * which is the reference's denormalize(distort(normalize(x))) then grid_sample's align_corners unnormalisation, in exact
 * arithmetic.  s: pinhole 1; simple_radial 1 + k1 r2; radial 1 + k1 r2 + k2 r2^2; simple_divisional
 * (1 - sqrt(max(0, 1 - 4 k1 r2))) / (2 k1 r2), 1 where k1 r2 = 0 -- evaluated as 2 / (1 + sqrt(t)) where t = 1 - 4 k1 r2 > 0
 * and 1 / (2 k1 r2) elsewhere, which does not cancel in float32 (the reference's form, which the LM solve keeps on purpose,
 * is off by 1.3 % at |k1 r2| = 1e-6).  Bilinear with zero padding, as F.grid_sample(bilinear, zeros, align_corners=True):
 * each of the four taps contributes only if it lies in [0, Win) x [0, Hin).  A non-finite coordinate (a NaN or inf in
 * the camera) contributes nothing: that output pixel is 0.  With s = 1, an exactly representable c and Win = W, H = Hin,
 * the output is a bit-exact copy.
 * Returns -3 (before any HIP call) for a NULL pointer, B, C, Hin or Win < 1, H or W < 2, H * W > 2^31 - 1,
 * cam_batch not 1 or B, a camera_model outside 0..3, B > 65535, or a destination that overlaps the source; -10 if the
 * launch fails.  Asynchronous on `stream`; no allocation.
 */
int gclm_undistort_image(int camera_model, const float* d_cam, int cam_batch, const float* d_src, int B, int C, int Hin,
                         int Win, int H, int W, float* d_dst, void* stream);

/*
 * BaseCamera.reproject_image / upright_image for a batch, in one pass: d_dst (B, C, H, W) is d_src (B, C, Hin, Win) as a
 * target camera, turned by a rotation, sees it; float32 NCHW.  d_src_cam and d_dst_cam are (cam_batch, 8)
 * {w, h, fx, fy, cx, cy, k1, k2} in device memory, the camera the image was taken with and the camera to render (the w, h
 * entries are not read: H, W are the output size, Hs, Ws the nominal size of the source camera, whose image may be stored at
 * another resolution Hin x Win, as for gclm_undistort_image); cam_batch applies to both: 1 shares one pair over the batch, B
 * gives each image its own.  d_rot is (rot_batch, 3, 3) row-major in device memory, rot_batch 1 or B, or NULL for the
 * identity (then rot_batch is still 1 or B).  For output pixel (x, y), integer pixel centres, no half-pixel offset:
 *   u = (x - cx_t) / fx_t,  v = (y - cy_t) / fy_t,  r2 = u^2 + v^2,  t = the TARGET model's undistort scale t(r2)
 *   q = (u t, v t, 1) M          (row vector times M, the convention of gclm_render_from_pano; M NULL: q = (u t, v t, 1))
 *   visible = q_z > 1e-3         (BaseCamera.eps, the reference's project())
 *   p = (q_x, q_y) / q_z,  r2s = |p|^2,  (s, s') = the SOURCE model's distort scale s(r2s) and ds/dr2
 *   inside_model = s + 2 r2s s' > 0
 *   ix = (p_x s fx_s + cx_s) (Win - 1) / (Ws - 1),   iy = (p_y s fy_s + cy_s) (Hin - 1) / (Hs - 1)
 * t as for gclm_render_from_pano, s as for gclm_undistort_image (the forms that do not cancel in float32); s': pinhole 0,
 * simple_radial k1, radial k1 + 2 k2 r2, simple_divisional 4 k1 / (sqrt(tau) (1 + sqrt(tau))^2) with tau = 1 - 4 k1 r2
 * (tau < 1e-6: the reference's expression at its clamp sqrt(1e-6)).  inside_model says that r s(r^2) still increases: beyond
 * that radius a polynomial model folds far rays back into the image.  Bilinear with zero padding, as
 * F.grid_sample(bilinear, zeros, align_corners=True); the output is exactly 0 where visible or inside_model fails and
 * where a coordinate is not finite.  A NaN or inf in a camera or in the rotation zeroes its whole image (an infinite q_z
 * counts as invisible).  d_valid (B, H, W) uint8, or NULL: 1 iff visible && inside_model && 0 <= ix <= Win - 1 &&
 * 0 <= iy <= Hin - 1.  With M the identity and the target the source's pinhole() this is gclm_undistort_image up to rounding.
 * Returns -3 (before any HIP call) for a NULL required pointer, a model outside 0..3, B outside 1..65535, C, Hin, Win, H or
 * W < 1, Hs or Ws < 2, H * W > 2^31 - 1 (or a tile grid of more than 2^32 threads), cam_batch or rot_batch not 1 or B, a
 * float pointer off a 4-byte boundary, or a destination or mask that overlaps any input or the other output; -10 if the
 * launch fails.  Asynchronous on `stream`; no allocation.
 */
int gclm_reproject_image(int src_model, const float* d_src_cam, int dst_model, const float* d_dst_cam, int cam_batch,
                         const float* d_rot, int rot_batch, const float* d_src, int B, int C, int Hin, int Win, int Hs, int Ws,
                         int H, int W, float* d_dst, unsigned char* d_valid, void* stream);

/*
 * gclm_undistort_image and gclm_reproject_image for uint8 images, planar or interleaved, in one pass: nothing is converted
 * before or after.  interleaved = 0: d_src (B, C, Hin, Win) and d_dst (B, C, H, W), one byte per element; interleaved = 1:
 * d_src (B, Hin, Win, C) and d_dst (B, H, W, C), C in 1..4 (torch: a channels_last (B, C, H, W) tensor).  Source and
 * destination share the layout; d_valid is (B, H, W) as for the float call.  Every other argument, the coordinates, the
 * visible and inside_model tests, the zero padding and the mask are those of gclm_undistort_image / gclm_reproject_image.  A
 * tap's byte is converted to float32 exactly, the sample is the float call's sum v00 w00 + v01 w01 + v10 w10 + v11 w11, and
 * the output byte is that sum rounded to nearest, ties to even, saturated to 0..255: 0 where the float call writes exactly
 * 0, and a byte-exact copy where the float call copies bit-exactly.
 * The byte pointers carry no alignment requirement (a frame cropped out of a larger buffer starts anywhere): interleaved
 * C = 4 images that both start on a 4-byte boundary are read and written as dwords, all others byte by byte, and the result
 * is the same bytes either way.
 * Returns -3 (before any HIP call) for everything the float call refuses -- its ranges counted in bytes, the image pointers
 * free of its 4-byte condition -- and for interleaved not 0 or 1, or interleaved = 1 with C > 4; -10 if the launch fails.
 * Asynchronous on `stream`; no allocation.
 */
int gclm_undistort_image_u8(int camera_model, const float* d_cam, int cam_batch, const unsigned char* d_src, int B, int C, int Hin,
                            int Win, int H, int W, int interleaved, unsigned char* d_dst, void* stream);
int gclm_reproject_image_u8(int src_model, const float* d_src_cam, int dst_model, const float* d_dst_cam, int cam_batch,
                            const float* d_rot, int rot_batch, const unsigned char* d_src, int B, int C, int Hin, int Win, int Hs,
                            int Ws, int H, int W, int interleaved, unsigned char* d_dst, unsigned char* d_valid, void* stream);

/*
 * get_up_field / get_latitude_field / get_perspective_field (geocalib/perspective_fields.py:47-74, 185-211, 278-320) for a
 * batch, in one pass that writes both fields: d_up (B, H, W, 2) interleaved and d_lat (B, H, W, 1) (the memory of
 * (B, 1, H, W)), float32; either may be NULL, not both.  d_cam is (B, 8) {w, h, fx, fy, cx, cy, k1, k2} and d_grav (B, 3)
 * {a, b, c} in device memory, one camera and one gravity per image (the w, h entries are not read: H, W are the size;
 * gravity is used as stored, not renormalised).  For pixel (x, y), integer pixel centres, no half-pixel offset:
 *   u = (x - cx) / fx,  v = (y - cy) / fy,  r2 = u^2 + v^2
 *   up:  p = (a - c u, b - c v),  q = s(r2) p + 2 s'(r2) (u, v) (u p_x + v p_y)      (pinhole: q = p)
 *        normalize_up = 1: up = q / max(|q|, 1e-12) (F.normalize);  normalize_up = 0: up = q
 *   lat: t = t(r2),  ray = (u t, v t, 1) / |(u t, v t, 1)|,  lat = asin(clamp(ray . (a, b, c), -1 + 1e-6, 1 - 1e-6))
 * s = the distort scale, s' = ds/dr2, t = the undistort scale: pinhole s = t = 1; simple_radial s = 1 + k1 r2, s' = k1,
 * t = 1 - k1 r2; radial s = 1 + k1 r2 + k2 r2^2, s' = k1 + 2 k2 r2, t = 1 - k1 r2 + (3 k1^2 - k2) r2^2; simple_divisional
 * t = 1 / (1 + k1 r2) (a zero denominator replaced by 1e6) and, with tau = 1 - 4 k1 r2, s = (1 - sqrt(max(0, tau))) /
 * (2 k1 r2), s' its derivative with sqrt(tau) clamped at 1e-3, both 1 and 0 where k1 r2 = 0 -- evaluated as s = 2 / (1 +
 * sqrt(tau)) (tau > 0) or 1 / (2 k1 r2) (tau <= 0) and s' = 4 k1 / (sqrt(tau) (1 + sqrt(tau))^2) (tau >= 1e-6), which do
 * not cancel in float32 (the reference's own evaluation does; below tau = 1e-6 its expression is used as written).
 * A NaN or inf in the camera or gravity gives NaN in the pixels where the reference's composition does.
 * Returns -3 (before any HIP call) for a NULL d_cam or d_grav, both outputs NULL, B outside 1..65535, H or W < 1,
 * H * W > 2^31 - 1 (or a grid of (W / 64) x (H / 4) tiles over 2^32 threads), a camera_model outside 0..3, normalize_up
 * not 0 or 1, a d_up not 8-byte or d_lat not 4-byte aligned, or an output that overlaps the other output, the camera or
 * the gravity; -10 if the launch fails.  Asynchronous on `stream`; no allocation.
 */
int gclm_perspective_fields(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W,
                            int normalize_up, float* d_up, float* d_lat, void* stream);

/*
 * The perspective fields of a calibration drawn over a batch of images, in one pass that reads a frame once and writes it
 * once: what the reference's demo shows (interactive_demo.py: plot_confidence, plot_latitude, draw_horizon_line,
 * plot_vector_field; viz2d.plot_perspective_fields), stated per output pixel and antialiased.  It is NOT cv2's rasteriser bit
 * for bit: end points are not truncated to integers, and the polylines of cv2.findContours are replaced by the distance to
 * the isoline.
 * gclm_draw_fields: d_src, d_dst (B, C, H, W) float32 planar, nominal range 0..1.  gclm_draw_fields_u8: bytes, interleaved = 0:
 * (B, C, H, W), interleaved = 1: (B, H, W, C) (torch: channels_last).  C is 3 or 4; channel 3 is copied.  d_cam (cal_batch, 8)
 * and d_grav (cal_batch, 3) as for gclm_perspective_fields, at the image's resolution, cal_batch 1 (shared) or B.  d_conf
 * (B, H, W) float32 or NULL.  d_palette, d_heat_palette: (256, 3) bytes in the image's channel order, or NULL where no layer
 * reads them.  `style` is host memory, read at call time.
 * One pixel at integer centre (x, y), float32 throughout; colours are 0..255 for byte images and bytes / 255 for float images.
 *   u, v, r2, t as for gclm_perspective_fields;  P = (u t, v t),  n = |(P, 1)|,  s = (P . (a, b) + c) / n,
 *   s_c = clamp(s, -1 + 1e-6, 1 - 1e-6),  lat = asin(s_c) 180 / pi                                    (degrees)
 *   grad_P s = ((a, b) - s P / n) / n,   dP/d(u, v) = t I + 2 t' (u, v)(u, v)^T,   d/dx = (d/du) / fx,  d/dy = (d/dv) / fy
 *   g = |grad_xy s| (180 / pi) / sqrt((1 - s_c)(1 + s_c))                                 (degrees of latitude per pixel)
 *   t' = dt/dr2: pinhole 0; simple_radial -k1; radial -k1 + 2 (3 k1^2 - k2) r2; simple_divisional -k1 t^2
 *   pal(L, tau), tau in [0, 1]: with i = min(floor(255 tau), 254) and f = 255 tau - i, L[i] + (L[i + 1] - L[i]) f
 * Layers, in this order, each out = out (1 - a) + colour a on channels 0..2:
 *   heat     (needs d_conf, d_heat_palette): tau = (clamp(log10(max(conf, 1e-6)), lo, hi) - lo) / (hi - lo), a = heat_alpha
 *   tint     (d_palette): tau = (lat + 90) / 180, a = tint_alpha
 *   contours (d_palette): step = 180 / (levels - 1), k = rint((lat + 90) / step), d = |lat - (-90 + k step)| / max(g, 1e-4),
 *            a = clamp(line_halfwidth + 0.5 - d, 0, 1), colour pal(palette, k / (levels - 1)); the level is evaluated as
 *            (2 k - (levels - 1)) 90 / (levels - 1), one rounding relative to the level and exact at the horizon
 *   horizon: a = clamp(line_halfwidth + 0.5 - |lat| / max(g, 1e-4), 0, 1), colour horizon_rgba
 *   arrows:  anchors (arrow_x0 + i S, arrow_y0 + j S), i, j >= 0, inside the image, S = arrow_step; q = the unnormalised up
 *            vector of gclm_perspective_fields at the anchor, e = q / |q|; the shaft runs from the anchor P0 to P1 = P0 + L e,
 *            two tip segments of length arrow_tip L from P1 along (-e +- e_perp) / sqrt 2 (45 degrees back towards P0); d = the
 *            distance from (x, y) to the nearest of the three segments, a = clamp(arrow_halfwidth + 0.5 - d, 0, 1), the largest
 *            over the anchors, colour arrow_rgba.  L + arrow_halfwidth + 0.5 <= S is a condition of the call, so only the four
 *            anchors of a pixel's cell can reach it.  An anchor with |q| < 1e-6 or a non-finite q draws nothing.
 * A non-finite lat (tint), lat or g (contours, horizon) or confidence (heat) skips that layer for that pixel: a NaN
 * calibration leaves the image unchanged.  With no layer on, the output is a byte-exact (float: bit-exact) copy.  The byte
 * written is the float rounded to nearest, ties to even, saturated to 0..255.
 * Returns -3 (before any HIP call) for a NULL d_cam, d_grav, d_src, d_dst or style, a model outside 0..3, B outside 1..65535,
 * C not 3 or 4, H or W < 1, H * W > 2^31 - 1 (or a tile grid over 2^32 threads), cal_batch not 1 or B, interleaved not 0 or 1,
 * a struct_size other than sizeof(gclm_overlay_style), unknown layer bits, an alpha outside [0, 1] or not finite, heat_hi <=
 * heat_lo or either not finite, levels < 2 (or even with the horizon layer on), a negative or non-finite half-width or arrow
 * length; with the arrow layer on: arrow_step < 1, a negative arrow_x0 or arrow_y0, arrow_tip outside [0, 1], or a violated
 * reach condition; a layer whose palette or confidence plane is NULL; a float pointer off a 4-byte boundary (byte images
 * carry no alignment requirement); or a destination that shares a byte with any range the call reads (drawing in place is
 * not supported).  -10 if the launch fails.  Asynchronous on `stream`; no allocation; one launch.
 */
enum gclm_overlay_layer {
    GCLM_OVERLAY_HEAT = 1, GCLM_OVERLAY_TINT = 2, GCLM_OVERLAY_CONTOURS = 4, GCLM_OVERLAY_HORIZON = 8, GCLM_OVERLAY_ARROWS = 16
};
typedef struct gclm_overlay_style {
    int32_t struct_size;             /* sizeof(gclm_overlay_style) of the CALLER's header */
    uint32_t layers;                 /* bit set of gclm_overlay_layer */
    float heat_alpha, tint_alpha;    /* in [0, 1] */
    float heat_lo, heat_hi;          /* range of log10(confidence) the heat palette spans */
    int32_t levels;                  /* latitude levels from -90 to 90 degrees, >= 2 */
    float line_halfwidth;            /* contours and horizon, pixels */
    int32_t arrow_step, arrow_x0, arrow_y0;
    float arrow_length, arrow_halfwidth, arrow_tip;
    unsigned char horizon_rgba[4], arrow_rgba[4];     /* channels 0..2 in the image's channel order; [3] is not read */
} gclm_overlay_style;
int gclm_draw_fields(int camera_model, const float* d_cam, const float* d_grav, int cal_batch, const float* d_src, int B, int C,
                     int H, int W, const float* d_conf, const unsigned char* d_palette, const unsigned char* d_heat_palette,
                     const gclm_overlay_style* style, float* d_dst, void* stream);
int gclm_draw_fields_u8(int camera_model, const float* d_cam, const float* d_grav, int cal_batch, const unsigned char* d_src, int B,
                        int C, int H, int W, int interleaved, const float* d_conf, const unsigned char* d_palette,
                        const unsigned char* d_heat_palette, const gclm_overlay_style* style, unsigned char* d_dst, void* stream);

/*
 * How well predicted perspective fields agree with a calibration, per image, in one pass over the planes: the reference's
 * up_error / latitude_error (siclib/models/utils/metrics.py:95-123) and the decoders' metrics built on them
 * (up_decoder.py:111-128, latitude_decoder.py:116-133), with the target fields of gclm_perspective_fields (normalize_up = 1)
 * at d_cam (B, 8) / d_grav (B, 3) evaluated per pixel in registers -- no target field is written or read.  Predictions in
 * the layout the solve takes: d_up (B, 2, H, W) planar, d_lat (B, 1, H, W), either may be NULL, not both; confidences
 * d_up_conf, d_lat_conf (B, H, W), either may be NULL.  All float32 in device memory; gravity is used as stored.
 * Per pixel, with t_up, t_lat the target:
 *   up:  e = deg(angle(p, t_up)) * mask.  The angle is acos(clamp(cosine_similarity(p, t_up), -1, 1)) with torch's
 *        eps = 1e-8, i.e. of P = p / max(|p|, eps) and T = t_up / max(|t_up|, eps), evaluated as atan2(|p x t|, p . t) where
 *        both norms reach eps and as atan2(sqrt((1 - |P|^2 |T|^2) + (P x T)^2), P . T) otherwise: forms that resolve small
 *        angles in float32, where acos of a cosine cannot (its smallest non-zero value is 0.02 degrees).
 *        mask = (p_x + p_y != 0) evaluated in float32, the reference's mask as written: a masked pixel has error 0 and is a
 *        hit at every threshold.
 *   lat: e = |lat - t_lat| * 180 / pi
 * NaN: a NaN prediction gives a NaN error (NaN * 0 stays NaN, as in torch); it makes that image's mean and weighted mean
 * of that field NaN and counts at no threshold; other images are untouched.
 * d_stats (B, S), S = 2 (2 + n_thresholds):  [up_mean, up_weighted, up_recall@t0 .., lat_mean, lat_weighted, lat_recall@t0 ..]
 *   mean = sum e / (H W) (all pixels, masked ones included);  weighted = sum(e conf) / sum conf (0 / 0 = NaN; NaN where that
 *   confidence is NULL);  recall@t = #(e < t) / (H W), strict;  the entries of a field whose pointer is NULL are NaN.
 * thresholds_deg is a HOST array of n_thresholds (0 .. GCLM_MAX_RECALL_THRESHOLDS) finite values in degrees, read before
 * the call returns.  Optional d_up_err, d_lat_err (B, H, W): the per-pixel errors (up_error * mask, latitude_error).
 * Every workgroup leaves one partial record (float32 sums, integer counts) in d_workspace, of at least
 * gclm_field_errors_workspace(B, H, W, n_thresholds) bytes (0 for sizes the call refuses); a second small launch sums each
 * image's records in float64 in a fixed order.  No atomics: results are bit-identical from call to call, and an image's
 * statistics do not depend on the other images of the batch (they depend on its pixels, H, W and on the planes' alignment:
 * four pixels per lane where W % 4 == 0 and every plane is 16-byte aligned, two where W is even and every plane 8-byte
 * aligned, one otherwise).
 * Returns -3 (before any HIP call) for a NULL d_cam, d_grav, d_stats or d_workspace, both fields NULL, a confidence or an
 * error map given for a NULL field, B outside 1..65535, H or W < 1, H * W > 2^31 - 1 (or a grid of (W / 64) x (H / 4) tiles
 * over 2^32 threads), a camera_model outside 0..3, n_thresholds outside 0..8, NULL thresholds with n_thresholds > 0, a
 * non-finite threshold, a workspace that is too small, a pointer that is not 4-byte aligned, or an output (statistics,
 * workspace, error maps) that overlaps an input or another output; -10 if a launch fails.  Asynchronous on `stream`; no
 * allocation.
 */
size_t gclm_field_errors_workspace(int B, int H, int W, int n_thresholds);
int gclm_field_errors(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, const float* d_up,
                      const float* d_lat, const float* d_up_conf, const float* d_lat_conf, int n_thresholds,
                      const float* thresholds_deg, void* d_workspace, size_t workspace_bytes, float* d_stats, float* d_up_err,
                      float* d_lat_err, void* stream);

/*
 * The losses the up and latitude heads are trained with, per image, and their gradients with respect to the predicted
 * fields: the reference's UpDecoder.calculate_losses / LatitudeDecoder.calculate_losses (siclib/models/decoders/
 * up_decoder.py:51-79, latitude_decoder.py:53-79), with the target fields of gclm_perspective_fields (normalize_up = 1) at
 * d_cam (B, 8) / d_grav (B, 3) evaluated per pixel in registers -- no target field is written or read, and nothing but the
 * inputs lives between the forward and the gradient call.  Planes as gclm_field_errors takes them: d_up (B, 2, H, W) planar,
 * d_lat (B, 1, H, W), either may be NULL, not both; confidences d_up_conf, d_lat_conf (B, H, W), either may be NULL -- a
 * NULL confidence is how a caller expresses use_uncertainty_loss = False.  All float32 in device memory; gravity is used as
 * stored.  Per pixel of a field, with r = p - t per component (up: 2, latitude: 1) and s = sum_c r_c^2:
 *   GCLM_FIELD_LOSS_L1      l = sum_c |r_c|                            dl/dp_c = sign(r_c), 0 at 0
 *   GCLM_FIELD_LOSS_L2      l = s                                      dl/dp_c = 2 r_c
 *   GCLM_FIELD_LOSS_DOT     l = 1 - sum_c r_c t_c  (up only; on the residual, as the reference writes it)   dl/dp_c = -t_c
 *   GCLM_FIELD_LOSS_CAUCHY  l = c^2 / 2 log1p(s / c^2), c = 0.007      dl/dp_c = r_c / (1 + s / c^2)
 *   GCLM_FIELD_LOSS_HUBER   l = sum_c h(r_c), delta = pi / 180 (nn.HuberLoss(delta=deg2rad(1))): h = r^2 / 2 for |r| < delta,
 *                           else delta (|r| - delta / 2)               dl/dp_c = clamp(r_c, -delta, delta)
 * gclm_field_loss: d_out (B, 4) = [up loss, latitude loss, up denominator, latitude denominator], loss = sum l / (H W) with
 * denominator H W, or sum(l conf) / sum conf with denominator sum conf where that confidence is given (the reference's
 * loss * (conf / sum conf * H W) followed by .mean()); no loss weight is applied; both entries of a NULL field are NaN.
 * sum conf = 0 gives NaN (0 / 0); a NaN prediction makes the loss of its image and field NaN and leaves the others untouched.
 * Every workgroup leaves one record of four float32 sums in d_workspace, of at least gclm_field_loss_workspace(B, H, W)
 * bytes (0 for sizes the call refuses); a second small launch sums each image's records in float64 in a fixed order.  No
 * atomics: results are bit-identical from call to call and do not depend on the other images of the batch (they depend on
 * the image's pixels, H, W and the pixels per lane, chosen as gclm_field_errors chooses them).
 * gclm_field_loss_grad: d_grad_up (B, 2, H, W) and d_grad_lat (B, 1, H, W), each given exactly when its field is:
 *   grad = d_scale[b, field] * dl/dp_c * (conf where that confidence is given),
 * d_scale (B, 2) = [up, latitude] in device memory, which the caller forms as grad_output * weight / denominator from d_out.
 * A NaN residual gives a NaN gradient at that pixel only (dot: -t_c does not depend on p); a NaN or zero-denominator scale
 * reaches every pixel of its image and field.  There is no gradient to the confidences; gclm_field_loss_param_grad, below, has
 * the gradients to the camera and the gravity.
 * Both return -3 (before any HIP call) for whatever gclm_field_errors refuses among the arguments they share (NULL d_cam or
 * d_grav, both fields NULL, a confidence given for a NULL field, B outside 1..65535, H or W < 1, H * W > 2^31 - 1 or a tile
 * grid over 2^32 threads, a camera_model outside 0..3), a loss id outside 0..4, GCLM_FIELD_LOSS_DOT for the latitude, a
 * pointer that is not 4-byte aligned, and an output that overlaps an input or another output; gclm_field_loss also for a
 * NULL d_out or d_workspace and a workspace that is too small; gclm_field_loss_grad also for a NULL d_scale, a gradient plane
 * given for a NULL field and a field without its gradient plane.  -10 if a launch fails.  Asynchronous on `stream`; no
 * allocation.
 */
enum gclm_field_loss {         /* (a tag: it shares no name space with the function below) */
    GCLM_FIELD_LOSS_L1 = 0,
    GCLM_FIELD_LOSS_L2 = 1,
    GCLM_FIELD_LOSS_DOT = 2,
    GCLM_FIELD_LOSS_CAUCHY = 3,
    GCLM_FIELD_LOSS_HUBER = 4
};
size_t gclm_field_loss_workspace(int B, int H, int W);
int gclm_field_loss(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, const float* d_up,
                    const float* d_lat, const float* d_up_conf, const float* d_lat_conf, int up_loss, int lat_loss,
                    void* d_workspace, size_t workspace_bytes, float* d_out, void* stream);
int gclm_field_loss_grad(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, const float* d_up,
                         const float* d_lat, const float* d_up_conf, const float* d_lat_conf, int up_loss, int lat_loss,
                         const float* d_scale, float* d_grad_up, float* d_grad_lat, void* stream);

/*
 * The loss the classification heads are trained with (the heads gclm_pack_fields_bins decodes), per image, and its gradient
 * with respect to the logits, against the calibration (camera rows, gravities) of each image: what a training step gets from
 * get_perspective_field + encode_up_bin / encode_bin_latitude + F.cross_entropy, with the target evaluated per pixel in
 * registers -- no field and no target map is rendered, no log-softmax of the logits' size is written; the logits are read
 * once forward and once more backward.
 * Logits as gclm_pack_fields_bins takes them: d_up_logits (B, up_bins, H, W) and d_lat_logits (B, lat_bins, H, W), planar, of
 * the one type logit_dtype (enum gclm_logit_dtype; 16-bit logits are the floats they widen to); either may be NULL, not both,
 * and an absent head's count is not looked at.  d_cam (B, 8), d_grav (B, 3) and the target fields as gclm_field_errors takes
 * and evaluates them (the up field normalised).  Confidences d_up_conf, d_lat_conf (B, H, W) float32, either may be NULL: a
 * NULL confidence is how a caller expresses use_uncertainty_loss = False.
 * Target bins, float32: up -- degrees = atan2(t_y, t_x) 180 / pi + 180, bin = rint(degrees / (360 / (up_bins - 1))) (half to
 * even), a full turn wraps to 0, a target that is exactly (0, 0) is the invalid class up_bins - 1; latitude -- class k holds
 * the degrees in (-90 + k 180 / lat_bins, -90 + (k + 1) 180 / lat_bins], the first and the last class open-ended.
 * Per pixel of a head with logits z and target bin t:  lse = log sum_k exp z_k,  ce = lse - z_t,  hit = [argmax_k z_k == t]
 * with torch.argmax's rule (the first index of the greatest value, a NaN above everything).
 * gclm_bin_loss writes
 *   d_out  (B, 6) float32 = [up numerator, up denominator, up hits, latitude numerator, latitude denominator, latitude hits]:
 *          numerator = sum w ce, denominator = sum w with w the head's confidence (H W, and w = 1, without one), hits = sum hit
 *          (exact below 2^24 pixels); the loss is numerator / denominator, the accuracy hits / (H W); no loss weight is applied;
 *          the three entries of a NULL head are NaN.  sum conf = 0 gives 0 / 0.
 *   d_lse  (B, 2, H, W) float32 and d_bins (B, 2, H, W) int16: lse and the target bin of every pixel, plane 0 the up head's,
 *          plane 1 the latitude's; the planes of a NULL head are not written.  gclm_bin_loss_grad reads them: the target is
 *          not evaluated a second time, so both passes agree on every pixel's bin.
 * Every workgroup leaves records of six float32 sums in d_workspace, of at least gclm_bin_loss_workspace(B, H, W) bytes (0 for
 * sizes the call refuses); a second small launch sums each image's records in float64 in a fixed order.  No atomics: results
 * are bit-identical from call to call, do not depend on the other images of the batch, and do not depend on the pixels per
 * lane (16-byte loads -- 4 float32 or 8 16-bit logits per lane -- where W is a multiple of that and every plane is 16-byte
 * aligned, else one pixel per lane: the same records either way).
 * gclm_bin_loss_grad writes d_grad_up (B, up_bins, H, W) and d_grad_lat (B, lat_bins, H, W) in the logits' type, rounded to
 * nearest even; either may be NULL, not both, and a head without its gradient is not read:
 *   grad[b, k] = d_scale[b, head] * w * (exp(z_k - lse) - [k == t]),
 * d_scale (B, 2) = [up, latitude] float32 in device memory, which the caller forms as grad_output * weight / denominator from
 * d_out.  There is no gradient to the confidences, the camera or the gravity: the targets are discrete.
 * Both return -3 (before any HIP call) for both logit tensors NULL, a confidence given for a NULL head, up_bins outside
 * 2..GCLM_MAX_BINS or lat_bins outside 1..GCLM_MAX_BINS (of a head that is given), an unknown logit_dtype, B < 0 or above
 * 65535, H or W < 1, H * W > 2^31 - 1 or a tile grid over 2^32 threads, a pointer that is not aligned to its element, and an
 * output that overlaps an input or another output; gclm_bin_loss also for a NULL d_cam, d_grav, d_workspace, d_out, d_lse or
 * d_bins, a camera_model outside 0..3 and a workspace that is too small; gclm_bin_loss_grad also for a NULL d_lse, d_bins or
 * d_scale, both gradients NULL and a gradient given for a NULL head.  B = 0 succeeds and launches nothing.  -10 if a launch
 * fails.  Asynchronous on `stream`; no allocation.
 */
size_t gclm_bin_loss_workspace(int B, int H, int W);
int gclm_bin_loss(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, const void* d_up_logits, int up_bins,
                  const void* d_lat_logits, int lat_bins, int logit_dtype, const float* d_up_conf, const float* d_lat_conf,
                  void* d_workspace, size_t workspace_bytes, float* d_out, float* d_lse, int16_t* d_bins, void* stream);
int gclm_bin_loss_grad(const void* d_up_logits, int up_bins, const void* d_lat_logits, int lat_bins, int logit_dtype,
                       const float* d_up_conf, const float* d_lat_conf, int B, int H, int W, const float* d_lse, const int16_t* d_bins,
                       const float* d_scale, void* d_grad_up, void* d_grad_lat, void* stream);

/*
 * The gradients of the same losses -- or of any function of the fields gclm_perspective_fields renders -- with respect to
 * the camera and the gravity the target fields are taken at, per image, in one pass over the planes and one small launch:
 * what the reference gets from autograd through get_perspective_field, with both fields rendered to memory and a dozen
 * eager kernels replayed backwards.  Per pixel the target t = (t_ux, t_uy, t_lat) is evaluated in registers by the renderer's
 * formulas in float64 from the float32 camera and gravity (a float32 target's rounding is 1e-5 of a typical residual and
 * would be the gradient's largest error), its cotangent g = (g_ux, g_uy, g_lat) is
 * formed, and g is pulled back in float64 to the entries the formulas of gclm_perspective_fields read -- gravity (a, b, c)
 * and camera fx, fy, cx, cy, k1, k2:
 *   up:   normalize: q-bar = (g - t (t . g)) / |q|  (|q| < 1e-12: q-bar = g / 1e-12, F.normalize's constant norm);  else q-bar = g
 *         q = s p + o (u, v), o = 2 s' D, D = u p_x + v p_y:   s-bar = q-bar . p,  o-bar = q-bar . (u, v),  s'-bar = 2 D o-bar,
 *         D-bar = 2 s' o-bar,  p-bar = s q-bar + D-bar (u, v),  (u, v)-bar = o q-bar + D-bar p
 *         p = (a - c u, b - c v):   a-bar += p-bar_x,  b-bar += p-bar_y,  c-bar -= p-bar . (u, v),  (u, v)-bar -= c p-bar
 *   lat:  inside the clamp  sl-bar = g_lat / sqrt(1 - sl^2),  beyond it 0;   sl = (X a + Y b + c) / N, N = |(X, Y, 1)|:
 *         a-bar += sl-bar X / N,  b-bar += sl-bar Y / N,  c-bar += sl-bar / N,  (X, Y)-bar = sl-bar ((a, b) - sl (X, Y) / N) / N
 *         (X, Y) = t (u, v):   (u, v)-bar += t (X, Y)-bar,  t-bar = (X, Y)-bar . (u, v)
 *   scales:  r2-bar = s-bar ds/dr2 + s'-bar ds'/dr2 + t-bar dt/dr2,  k-bar = s-bar ds/dk + s'-bar ds'/dk + t-bar dt/dk, with the
 *         partial derivatives of the forms above (simple_divisional, E = sqrt(tau) (1 + sqrt(tau))^2:  ds/dk1 = 4 r2 / E,
 *         ds'/dk1 = 4 / E + 16 k1 r2 E_tau / E^2,  ds'/dr2 = 16 k1^2 E_tau / E^2,  E_tau = (1 + sqrt(tau)) (1 + 3 sqrt(tau)) /
 *         (2 sqrt(tau));  dt/dk1 = -r2 t^2,  dt/dr2 = -k1 t^2;  at k1 r2 = 0: s = 1, s' = 0 are constants)
 *         r2 = u^2 + v^2:   (u, v)-bar += 2 r2-bar (u, v)
 *   u = (x - cx) / fx:   fx-bar = -u-bar u / fx,  cx-bar = -u-bar / fx,  and likewise fy, cy from v-bar.
 * The derivative is that of the branch the renderer takes, its conditions constants.  The conditions of the distort and
 * undistort scales (tau, k1 r2 = 0, a zero denominator) are evaluated on the renderer's own float32 u, r2; every other one --
 * the latitude's clamp, the 1e-12 norm floor, huber's delta, l1's sign -- on the float64 values, while gclm_field_loss decides
 * them on its float32 target: for a value within about 1e-7 of a branch point the gradient's branch can differ from the
 * forward's.  A lane sums its pixels in float64 (the
 * terms of a parameter cancel across the image); every workgroup leaves one record of nine float64 sums in d_workspace, of
 * at least gclm_field_param_grad_workspace(B, H, W) bytes (0 for sizes the calls refuse), 8-byte aligned; the second launch
 * sums each image's records in a fixed order.  No atomics, no memset: results are bit-identical from call to call, do not
 * depend on the other images of the batch nor on which of the two outputs is asked for (they depend on the image, H, W and
 * the pixels per lane: two where W is even and every plane is 8-byte aligned, the interleaved up cotangent 16-byte; one
 * otherwise).
 * Outputs: d_grad_cam (B, 8) in the layout of d_cam -- columns w, h are written as 0, k2's column is 0 for the
 * one-parameter models and both distortion columns for pinhole -- and d_grad_grav (B, 3); either may be NULL, not both.
 * gclm_field_loss_param_grad: the cotangent comes from the loss,  g_c = d_scale[b, field] * conf * dl/dt_c  with the planes,
 *   loss ids and d_scale of gclm_field_loss_grad (normalize_up = 1);  dl/dt_c = -dl/dp_c for l1, l2, cauchy and huber;  for dot,
 *   l = 1 - sum_c (p_c - t_c) t_c, so dl/dt_c = 2 t_c - p_c.  The confidence normalisation is detached, as in the forward.
 * gclm_perspective_fields_backward: the cotangent is read from planes in the layout gclm_perspective_fields writes, d_grad_up
 *   (B, H, W, 2) interleaved and d_grad_lat (B, H, W); either may be NULL, not both.
 * Both return -3 (before any HIP call) for a NULL d_cam, d_grav or d_workspace, both outputs NULL, B outside 1..65535, H or
 * W < 1, H * W > 2^31 - 1 or a tile grid over 2^32 threads, a camera_model outside 0..3, a workspace that is too small or not
 * 8-byte aligned, a pointer that is not 4-byte aligned, and an output or the workspace overlapping an input or each other;
 * gclm_field_loss_param_grad also for whatever gclm_field_loss_grad refuses among the arguments they share (both fields NULL,
 * a confidence given for a NULL field, a loss id outside 0..4, GCLM_FIELD_LOSS_DOT for the latitude, a NULL d_scale);
 * gclm_perspective_fields_backward also for both cotangent planes NULL, normalize_up not 0 or 1 and a d_grad_up that is not
 * 8-byte aligned.  -10 if a launch fails.  Asynchronous on `stream`; no allocation.
 */
size_t gclm_field_param_grad_workspace(int B, int H, int W);
int gclm_field_loss_param_grad(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, const float* d_up,
                               const float* d_lat, const float* d_up_conf, const float* d_lat_conf, int up_loss, int lat_loss,
                               const float* d_scale, void* d_workspace, size_t workspace_bytes, float* d_grad_cam,
                               float* d_grad_grav, void* stream);
int gclm_perspective_fields_backward(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, int normalize_up,
                                     const float* d_grad_up, const float* d_grad_lat, void* d_workspace, size_t workspace_bytes,
                                     float* d_grad_cam, float* d_grad_grav, void* stream);

/*
 * Which of N candidate calibrations per image fits the image's predicted perspective fields best, in one pass over the
 * planes: the scores the reference's RANSAC baseline ranks its hypotheses with (siclib/models/optimization/ransac.py:
 * check_up_inliers, check_latitude_inliers, get_best_index), with every hypothesis' target fields evaluated per pixel in
 * registers -- no field is rendered, and each plane of an image is read once per GCLM_HYPOTHESIS_CHUNK hypotheses.
 * Predictions as gclm_field_errors takes them: d_up (B, 2, H, W) planar, d_lat (B, 1, H, W), either may be NULL, not both;
 * confidences d_up_conf, d_lat_conf (B, H, W), either may be NULL: a NULL confidence counts as 1.  Optional d_mask (B, H, W)
 * multiplies both contributions (the reference's `inliers`; usually zeros and ones, any weight is taken as it is).
 * d_cam (B, N, 8), d_grav (B, N, 3): hypothesis n of image b is row b N + n, the reference's (B N) order; one camera model
 * per call; gravity is used as stored.  All float32 in device memory.
 * Per pixel and hypothesis, e_up and e_lat are exactly the per-pixel errors of gclm_field_errors at that hypothesis (the
 * normalised target, the masked atan2 angle in degrees, |lat - t_lat| 180 / pi).  Then, with c the confidence times the mask,
 *   up[b, n]    = sum over pixels of (e_up < up_threshold_deg ? 1 : 0) * c_up,   strict;   lat[b, n] likewise
 *   total[b, n] = up_weight up[b, n] + lat_weight lat[b, n]
 * d_scores (B, N, 3) = [up, lat, total]; the scores of a field whose pointer is NULL are 0 (the reference returns zeros for
 * an absent latitude).  Optional d_best (B) int32: the first index of the largest total of that image, compared on the
 * float32 totals as written; a NaN total counts as the maximum, as torch.argmax has it.
 * hit * c is a multiplication, as in torch: a NaN error (a NaN prediction, a NaN in the hypothesis' camera or gravity) hits
 * nothing and contributes 0 -- such a hypothesis scores 0 and is no error; a NaN confidence or mask pixel makes that field's
 * score of that image NaN for EVERY hypothesis (an infinite one: NaN for the hypotheses that miss the pixel) and leaves the
 * other images untouched.  The thresholds (degrees) and weights are host floats, finite.
 * Every workgroup scores one tile of pixels against one chunk of hypotheses and leaves one partial record (float32 sums)
 * per hypothesis in d_workspace, of at least gclm_hypothesis_scores_workspace(B, N, H, W) bytes (0 for sizes the call
 * refuses); a second small launch sums each hypothesis' records in float64 in a fixed order, forms total in float64, rounds
 * once and takes the argmax.  No atomics: results are bit-identical from call to call, and the bits of d_scores[b, n]
 * depend on image b's pixels, H, W, the planes' alignment (pixels per lane, as gclm_field_errors: four where W % 4 == 0 and
 * every plane is 16-byte aligned, two where W is even and every plane 8-byte aligned, one otherwise) and the eleven
 * numbers of hypothesis (b, n) alone -- not on N, on n, on the other hypotheses or on the other images.
 * Returns -3 (before any HIP call) for a NULL d_cam, d_grav, d_scores or d_workspace, both fields NULL, a confidence given
 * for a NULL field, B or N outside 1..65535, H or W < 1, H * W > 2^31 - 1 (or a grid of (W / 64) x (H / 4) tiles over 2^32
 * threads), a camera_model outside 0..3, a non-finite threshold or weight, a workspace that is too small, a pointer that is
 * not 4-byte aligned, or an output (scores, best, workspace) that overlaps an input or another output; -10 if a launch
 * fails.  Asynchronous on `stream`; no allocation.
 */
size_t gclm_hypothesis_scores_workspace(int B, int N, int H, int W);
int gclm_hypothesis_scores(int camera_model, const float* d_cam, const float* d_grav, int B, int N, int H, int W,
                           const float* d_up, const float* d_lat, const float* d_up_conf, const float* d_lat_conf,
                           const float* d_mask, float up_threshold_deg, float lat_threshold_deg, float up_weight,
                           float lat_weight, void* d_workspace, size_t workspace_bytes, float* d_scores, int* d_best,
                           void* stream);

/*
 * The three-pixel minimal solver of the reference's RANSAC baseline (siclib/models/optimization/ransac.py: MinimalSolver,
 * RPFSolver.solve_rpf), one lane per sample: N samples per image give the N Rn candidate calibrations that
 * gclm_hypothesis_scores ranks.  Pinhole, square pixels, principal point (c_x, c_y) = (W / 2, H / 2); integer pixel centres.
 * d_up (B, 2, H, W) planar and d_lat (B, 1, H, W) in radians as gclm_hypothesis_scores takes them; d_prior_focal (B) or NULL;
 * d_lat may be NULL only with d_prior_focal (the latitude is then not read).  Rn = 2 without a prior focal, 1 with one.
 * d_samples (B, N, 3, 2) int32 = (x_k, y_k), k = 0, 1, 2, or NULL: the pixels are then drawn in the kernel (below).
 * Per sample, all in float32, no fused multiply-adds:
 *   1. d_k = d_up[b, :, y_k, x_k], k = 0, 1.  l_k = (-d_ky, d_kx, x_k d_ky - y_k d_kx), V = l_0 x l_1 (homogeneous, never
 *      divided by V_z), v = (V_x - c_x V_z, V_y - c_y V_z, V_z) / |.|.
 *   2. U = x_2 - c_x, Vp = y_2 - c_y, L = sin(d_lat[b, y_2, x_2]), R = U^2 + Vp^2, S = v_x^2 + v_y^2, D = v_x U + v_y Vp.
 *   3. a0 = (L^2 - 1) v_z^2, a1 = L^2 (R v_z^2 + S) - 2 D v_z, a2 = L^2 R S - D^2;  q = -(a1 + sgn(a1) sqrt(a1^2 - 4 a0 a2)) / 2
 *      (sgn(0) = 1); F_0 = a2 / q, F_1 = q / a0.  With a prior focal: the one root F_0 = prior^2.
 *   4. Per root r: f = sqrt(F_r), g = normalize(v_x / f, v_y / f, v_z), negated if
 *      (g_x - g_z (x_0 - c_x) / f) d_0x + (g_y - g_z (y_0 - c_y) / f) d_0y < 0: the up direction at pixel 0 decides the sign.
 *   5. The row is valid iff f and g are finite, H / 2 / tan 75 deg <= f <= H / 2 / tan 2.5 deg (the solve's own focal
 *      clamp, as float32 constants: H 0.5 / 3.7320504, H 0.5 / 0.043660942) and, without a prior focal,
 *      L (g_x U / f + g_y Vp / f + g_z) >= 0 (the root that squaring introduced fails this).
 *   6. Row n Rn + r of image b: d_cam = {W, H, f, f, W / 2, H / 2, 0, 0}, d_grav = g; an invalid row holds eleven NaNs, which
 *      gclm_hypothesis_scores scores exactly 0.  Identical pixels 0 and 1, parallel up vectors that meet nowhere finite in
 *      float32, a NaN among the values read and a negative discriminant all end in an invalid row, never in an error.
 * The draw (d_samples == NULL): with mix(z) the splitmix64 finaliser -- z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) *
 * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31, all modulo 2^64 -- and i = first_index + b,
 *   base = mix((seed ^ GCLM_RPF_DRAW_SALT) ^ mix(i * 0xD1342543DE82EF95 + 1)),   h = mix(base + 4 n + k),
 *   x_k = ((h >> 32) * W) >> 32,   y_k = ((h & 0xFFFFFFFF) * H) >> 32:
 * a function of (seed, first_index + b, n, k), W and H alone, so image b alone with first_index advanced by b draws the
 * same pixels.  Optional d_samples_out (B, N, 3, 2) int32 receives the pixels used, drawn or given.
 * The samples live in device memory, so the host cannot check them: a sample with a coordinate outside [0, W) x [0, H) reads
 * nothing and leaves invalid rows (the Python package refuses such samples before the call).
 * One launch, grid (ceil(N / 256), B); no LDS, no atomics, no workspace: the rows of sample (b, n) depend on that sample's
 * three pixels alone, and two calls give the same bits.
 * Returns -3 (before any HIP call) for a NULL d_up, d_cam or d_grav, a NULL d_lat without d_prior_focal, B outside 1..65535,
 * N outside 1..GCLM_RPF_MAX_SAMPLES, H or W < 1, H * W > 2^31 - 1, a pointer that is not 4-byte aligned, or an output (d_cam,
 * d_grav, d_samples_out) that overlaps an input or another output; -10 if the launch fails.  Asynchronous on `stream`; no
 * allocation.
 */
int gclm_rpf_hypotheses(const float* d_up, const float* d_lat, const float* d_prior_focal, const int32_t* d_samples,
                        uint64_t seed, int64_t first_index, int B, int N, int H, int W, float* d_cam, float* d_grav,
                        int32_t* d_samples_out, void* stream);

/*
 * The reference's THIRD optimiser beside the LM and the RANSAC baseline (siclib/models/optimization/perspective_opt.py:
 * PerspectiveParamOpt): Adam on (roll, pitch, vfov) of a pinhole camera, per image, against predicted fields d_up (B,2,H,W)
 * planar and d_lat (B,1,H,W), float32.  The reference takes one image per call, renders both fields and runs autograd each
 * step; here a step is one pass over the three planes and one small launch for the whole batch, and every image is its own
 * reference call: own Adam moments, own learning rate, own stop.
 *
 * Per image the state is (r, p, v); g = (-sin r cos p, -cos r cos p, sin p), f = (H / 2) / tan(v / 2), fx = fy = f, principal
 * point (W / 2, H / 2), integer pixel centres.  With the predicted fields of that camera (gclm_perspective_fields' formulas),
 * means over H * W:
 *   up  = mean acos(clip(cos_sim(up_pred, t), -1 + 1e-7, 1 - 1e-7)),   cos_sim as torch: t / max(|t|, 1e-8)
 *   lat = mean |lat_pred - l|
 *   total = lamb * lat + (1 - lamb) * up, formed in float64 from the two float32 means and rounded once to float32.
 * The angle is evaluated as atan2(|U x T|, U . T) held to [theta_clip, pi - theta_clip], theta_clip = acos(1 - 1e-7) -- the
 * same function, but small angles resolve in float32 -- and the gradient in closed form, without autograd and without a
 * division by sin of the angle: d angle / ds = -sign(U x T) (n . dq/ds) / |q| with q the unnormalised up, n = (-U_y, U_x); 0
 * where the clip is active.  Latitude: sign(lat_pred - l) ds / sqrt(1 - s^2), s the sine under the asin, 0 where its clamp
 * (gclm_perspective_fields') is active.  (r, p) enter by the tangent columns of Gravity.J_rp, v by df/dv = -(H / 4) / sin^2(v / 2).
 *
 * gclm_param_opt_cost: ONE evaluation at given parameters d_rpv (B,3): d_out (B,8) = [up, lat, d up / d(r, p, v),
 * d lat / d(r, p, v)].  Three launches (pose records, the pass, the per-image sums).
 *
 * gclm_param_opt_step: ONE update of B state records d_state from d_cost (B,8) as above -- the stage entry of the loop's
 * update, in the reference's order: the Adam step, then the scheduler's step on the loss, then check_convergence on the same
 * loss.  A state record is GCLM_PARAM_OPT_STATE_WORDS 32-bit words, 8-byte aligned:
 *   0..2  float   roll, pitch, vfov            9  int32  steps taken (Adam's t)     14..15 double  learning rate
 *   3..5  float   Adam's first moments        10  int32  converged (0 / 1)          16     float   scheduler's best
 *   6..8  float   Adam's second moments       11  int32  scheduler's num_bad_epochs 17..19 float   last total, up, lat
 *                                             12  int32  scheduler's cooldown count 20..27 float   the window of losses
 *                                             13  int32  losses in the window       28..31 (the loop: initial r, p, v; else 0)
 * A fresh record holds the parameters, the learning rate, best = +inf and zeros.  A record whose converged word is set is
 * left as it is.
 *   Adam: torch's defaults, betas (0.9, 0.999), eps 1e-8, bias corrections, gradient = float32(lamb * d lat + (1 - lamb) * d up);
 *     parameters and moments are float32, one step's arithmetic is float64 and each is rounded once.
 *   Scheduler (use_scheduler != 0): torch's ReduceLROnPlateau, mode "min", threshold_mode "rel": loss < best * (1 -
 *     sched_threshold) sets best and zeroes num_bad_epochs, anything else (a NaN too) counts one; a running cooldown counts down and
 *     zeroes num_bad_epochs; num_bad_epochs > sched_patience sets lr = max(lr * sched_factor, sched_min_lr) if that lowers it by
 *     more than sched_eps, starts the cooldown and zeroes num_bad_epochs.
 *   check_convergence, in this order: loss <= abs_tol stops; a window of fewer than `patience` losses appends the loss;
 *     |loss - window[0]| < rel_tol stops; otherwise the loss is appended and the last `patience` are kept.
 *   Every comparison is made in float64 on the float32 loss (Python's .item()).  The step that detects convergence has
 *   applied its Adam update.  Nothing clamps vfov.  A NaN loss never converges.
 *
 * gclm_param_opt: the loop.  d_init_rpv (B,3), or NULL for the reference's _get_init_params: roll = -atan2(up_x, -up_y) and
 * pitch = latitude at pixel (H / 2, W / 2) (integer division), vfov = |lat[0, W / 2] - lat[H - 1, W / 2]| held to [20, 120]
 * degrees -- read back, as the reference reads them, from the Gravity and the camera built of them (Gravity.roll's 1e-4 in
 * the denominator included).  Up to max_steps steps of pass + update; an image that has converged freezes and its workgroups
 * return after one load.  d_rpv (B,3) receives the parameters, d_info (B, GCLM_PARAM_OPT_INFO_WORDS) floats:
 *   [0] steps taken  [1] converged (0 / 1)  [2..4] total, up, lat of the last evaluation (at the parameters BEFORE the last
 *   update, as the reference's last loss)  [5] final learning rate  [6..8] the initial (r, p, v)  [9..11] 0.
 * poll_every = 0 enqueues all max_steps steps without a host synchronisation; poll_every = n > 0 reads the count of
 * converged images back every n steps -- a synchronisation of `stream` the caller asked for -- and stops enqueueing once no
 * image is live.  The results are bit-identical either way, and an image's bits depend on its own pixels, H, W and the
 * alignment of the planes alone (4 pixels per lane where W % 4 == 0 and both planes are 16-byte aligned, 2 where W is even and
 * both 8-byte aligned, else 1; the three paths agree to float32 rounding of a pixel's terms and the order of the sums), not on B or
 * the other images.
 *
 * The caller owns the workspace: gclm_param_opt_workspace(B, H, W) bytes (0 for sizes the calls refuse), 16-byte aligned, for
 * gclm_param_opt and gclm_param_opt_cost alike.  gclm_default_param_opt_config fills the reference's default_conf (max_steps
 * 1000, lr 0.01, patience 3, abs_tol 1e-7, rel_tol 1e-9, lamb 0.5, ReduceLROnPlateau with patience 3 and torch's other
 * defaults: factor 0.1, threshold 1e-4, cooldown 0, min_lr 0, eps 1e-8), poll_every 16 and struct_size.
 * All three calls return -3 (before any HIP call) for a NULL pointer (d_init_rpv may be NULL), B outside 1..65535, H or W < 2,
 * H * W > 2^31 - 1, a pointer off its alignment (4 bytes; d_state 8; the workspace 16), an output that overlaps an input, the
 * workspace or another output, a workspace smaller than gclm_param_opt_workspace says, or a config with a wrong struct_size,
 * max_steps outside 1..GCLM_PARAM_OPT_MAX_STEPS, patience outside 1..GCLM_PARAM_OPT_MAX_PATIENCE, lr negative or not finite,
 * lamb outside [0, 1], a NaN tolerance, sched_patience, sched_cooldown or poll_every < 0, sched_factor outside [0, 1),
 * sched_threshold, sched_min_lr or sched_eps negative or not finite; -10 if a launch fails.  Asynchronous on `stream` (but for the
 * polls); no allocation.
 */
#define GCLM_PARAM_OPT_STATE_WORDS 32
#define GCLM_PARAM_OPT_INFO_WORDS 12
#define GCLM_PARAM_OPT_MAX_PATIENCE 8
#define GCLM_PARAM_OPT_MAX_STEPS 1000000
typedef struct gclm_param_opt_config {
    int32_t struct_size;        /* sizeof(gclm_param_opt_config) */
    int32_t max_steps;
    int32_t patience;           /* check_convergence's window */
    int32_t use_scheduler;      /* 0: lr_scheduler.name = None */
    int32_t sched_patience;
    int32_t sched_cooldown;
    int32_t poll_every;
    int32_t reserved;           /* 0 */
    double lr, abs_tol, rel_tol, lamb;
    double sched_factor, sched_threshold, sched_min_lr, sched_eps;
} gclm_param_opt_config;
int gclm_default_param_opt_config(gclm_param_opt_config* config);
size_t gclm_param_opt_workspace(int B, int H, int W);
int gclm_param_opt_cost(const float* d_up, const float* d_lat, const float* d_rpv, int B, int H, int W, void* d_workspace,
                        size_t workspace_bytes, float* d_out, void* stream);
int gclm_param_opt_step(void* d_state, const float* d_cost, int B, const gclm_param_opt_config* config, void* stream);
int gclm_param_opt(const float* d_up, const float* d_lat, const float* d_init_rpv, int B, int H, int W,
                   const gclm_param_opt_config* config, void* d_workspace, size_t workspace_bytes, float* d_rpv, float* d_info,
                   void* stream);

/*
 * BaseCamera.get_img_from_pano (geocalib/camera.py:414-514) for n images, in one pass: d_dst (n, C, H, W) holds image i
 * rendered from the equirectangular panorama srcs[i] (C, Hs, Ws) with Hs = src_hw[2 i], Ws = src_hw[2 i + 1], float32
 * NCHW.  srcs and src_hw are HOST arrays of n device pointers and 2 n sizes (a pointer may repeat: n images of one
 * panorama).  d_cam is (cam_batch, 8) {w, h, fx, fy, cx, cy, k1, k2} in device memory (the w, h entries are not read: H, W
 * are the output size); cam_batch = 1 shares one camera over the batch, cam_batch = n gives each image its own.  d_rot is
 * (n, 3, 3) row-major in device memory: R_i = gravity.R[i] @ rad2rotmat(0, 0, yaw_i).  For output pixel (x, y), integer
 * pixel centres, no half-pixel offset:
 *   u = (x - cx) / fx,  v = (y - cy) / fy,  r2 = u^2 + v^2,  t = the model's undistort scale t(r2)
 *   q = (u t, v t, 1) R_i,  lon = atan2(q_x, q_z),  lat = atan2(q_y, hypot(q_x, q_z))
 *   ix = (lon / pi + 1) / 2 (Ws - 1),   iy = (2 lat / pi + 1) / 2 (Hs - 1)
 * t: pinhole 1; simple_radial 1 - k1 r2; radial 1 - k1 r2 + (3 k1^2 - k2) r2^2; simple_divisional 1 / (1 + k1 r2), with a
 * zero denominator replaced by 1e6.  The reference normalises (u t, v t, 1) first; both angles are invariant to that scale.
 * Bilinear with zero padding, as F.grid_sample(bilinear, zeros, align_corners=True): each of the four taps contributes
 * only if it lies in [0, Ws) x [0, Hs); longitude does not wrap at +-pi.  A non-finite coordinate (a NaN or inf in the
 * camera or the rotation) contributes nothing: that output pixel is 0.
 * Returns -3 (before any HIP call) for a NULL pointer (srcs[i] included), n outside 1..65535, C < 1, H or W < 2,
 * H * W > 2^31 - 1, any Hs or Ws < 2, cam_batch not 1 or n, a camera_model outside 0..3, or a destination that overlaps a
 * source, the camera or the rotations; -10 if a launch fails.  Asynchronous on `stream` (one launch per 192 images); no
 * allocation, no host-to-device copy: the panorama table travels in the kernel arguments.
 */
int gclm_render_from_pano(int camera_model, const float* d_cam, int cam_batch, const float* d_rot, const float* const* srcs,
                          const int* src_hw, int n, int C, int H, int W, float* d_dst, void* stream);

/*
 * LMOptimizer.calculate_gradient_and_hessian (geocalib/lm_optimizer.py:317-385) on materialised tensors:
 *   d_G (B,P) = sum_px w J^T r,   d_H (B,P,P) = sum_px w J^T J
 * for d_J (B,N,R,P), d_residual (B,N,R), d_weight (B,N); R rows per pixel (2 for the up field, 1 for latitude).
 * `accumulate` != 0 adds to the existing d_G / d_H (up + latitude, :444-459).  The solve itself never forms J
 * (gclm_solve contracts it in registers); this serves callers that hold the tensors.
 */
int gclm_gradient_hessian(const float* d_J, const float* d_residual, const float* d_weight, int B, int N, int R,
                          int P, int accumulate, float* d_G, float* d_H, void* stream);

/*
 * optimizer_step (geocalib/lm_optimizer.py:109-137) for B systems of P <= 5 unknowns, on the device:
 *   delta = (H + diag(clamp(lambda * diag(H), min = eps)))^-1 G        (fp32 Cholesky per system)
 * d_G (B,P), d_H (B,P,P), d_lambda (B) or one value (lambda_is_scalar), d_delta (B,P).  A system that is not
 * positive definite gets delta = 0 and d_failed[b] = 1 (d_failed may be NULL); the reference moves H and G to the
 * CPU for this step and zeroes the whole batch on a failure.
 */
int gclm_optimizer_step(const float* d_G, const float* d_H, const float* d_lambda, int lambda_is_scalar, float eps,
                        int B, int P, float* d_delta, int* d_failed, void* stream);

/*
 * LMOptimizer.calculate_residuals (geocalib/lm_optimizer.py:248-274) as one launch: per-pixel residuals of the
 * fields against the prediction of (d_cam (B,8), d_grav (B,3)):  d_r_up (B,H*W,2) = up_data - up(theta),
 * d_r_lat (B,H*W,1) = sin(lat_data) - sin(lat(theta)).  Either output may be NULL (then its field may be NULL).
 */
int gclm_residual_fields(int camera_model, const float* d_up, const float* d_lat, const float* d_cam,
                         const float* d_grav, int B, int H, int W, float* d_r_up, float* d_r_lat, void* stream);

/*
 * LMOptimizer.calculate_costs (geocalib/lm_optimizer.py:276-315) for one residual tensor: n rows of `dim`
 * components (dim = 0: the n inputs already are |r|^2) -> scaled Huber cost and weight at `scale` (scaled_loss
 * :61-76, huber_loss :79-87), both multiplied by d_conf (n) when given, and the scaled loss's second derivative,
 * which is NOT multiplied by d_conf (scaled_loss's d2 carries no confidence).  The weight is floored at FLT_EPSILON
 * as the reference's is (y = |r|^2 / scale^2 beyond 1/eps^2); y = +inf gives cost inf, weight eps, second -0.
 * d_cost / d_weight / d_second (n) may each be NULL.
 */
int gclm_huber_costs(const float* d_residual, size_t n, int dim, float scale, const float* d_conf, float* d_cost,
                     float* d_weight, float* d_second, void* stream);

/*
 * The reference's J_perspective_field (geocalib/perspective_fields.py:323-365 -> J_up_field :84-182,
 * J_latitude_field :214-275) as one launch: per-pixel Jacobians of the PREDICTED up / latitude fields of B cameras
 * wrt (delta_1, delta_2, focal[, k1[, k2]]).  d_cam (B,8), d_grav (B,3) as in gclm_solve; spherical / log_focal
 * select the tangent basis (SphericalManifold.J_plus vs Gravity.J_rp) and the focal parametrisation exactly as
 * the reference's flags.  Outputs (either may be NULL): d_J_up (B,H,W,2,P), d_J_lat (B,H,W,1,P) with
 * P = 3 + number of distortion parameters of `camera_model`.  A solve never materialises these (the sweep
 * contracts them in registers); this entry point exists for callers and tests that want the fields themselves.
 */
int gclm_jacobian_fields(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W,
                         int spherical, int log_focal, float* d_J_up, float* d_J_lat, void* stream);

/*
 * Measurement helper (bench.py, tests): synthetic perspective fields generated on the device,
 * SURVEY.md section 8(d).  Image i depends on (seed, first_index + i) only, so every sharding of
 * a batch sees identical data.  Writes the 5 planes and the ground truth (B,8) / (B,3).
 */
int gclm_synth_fields(int camera_model, uint64_t seed, int64_t first_index, int B, int H, int W,
                      float noise_sigma, float* d_up, float* d_lat, float* d_up_conf,
                      float* d_lat_conf, float* d_gt_cam, float* d_gt_grav, void* stream);

/* Same generator with shared-intrinsics structure and strided index runs (multi-GPU frame split):
 * intrinsics (focal, k1) are keyed by global_index / group_size (group_size <= 1: per image), and local
 * image b maps to global index first_index + (b / run) * run_stride + b % run (run = 0: contiguous). */
int gclm_synth_fields_grouped(int camera_model, uint64_t seed, int64_t first_index, int B, int H, int W,
                              float noise_sigma, int group_size, int run, int run_stride, float* d_up,
                              float* d_lat, float* d_up_conf, float* d_lat_conf, float* d_gt_cam,
                              float* d_gt_grav, void* stream);

/*
 * Measurement helper (bench.py: roofline.read_ceiling_frac; no reference counterpart): ONE launch that streams n_planes
 * (<= 8) device planes of `floats` floats each (16-byte aligned, floats % 4 == 0) with the sweep's own load -- non-temporal,
 * 16 bytes per lane, consecutive lanes on consecutive addresses, four loads per plane in flight per thread -- and no
 * arithmetic beyond the sum that keeps the loads alive.  Its duration is what THESE buffers can stream on THIS box: the
 * memory-system ceiling of the sweep's access pattern for the allocation a measurement was taken on.  d_planes is a HOST
 * array of device pointers.  Asynchronous on `stream`; the caller times it (events on that stream).
 */
int gclm_read_probe(const float* const* d_planes, int n_planes, size_t floats, void* stream);

/*
 * Multi-GPU collectives over RCCL / xGMI, one process per GPU (no reference counterpart: the
 * reference's LM is single-process).  gclm_comm_unique_id is called on rank 0 only and its 128 bytes are handed to
 * the other ranks by the caller.  Both collectives are asynchronous on `stream`.
 *   gclm_comm_all_gather      the ONE gather of packed result rows (configs[2]); recv holds nranks * count floats
 *   gclm_comm_all_reduce_sum  the ONE in-place sum of the (num_groups x GCLM_SHARED_PARTIAL_STRIDE) Schur partials
 *                             per LM step between gclm_shared_reduce and gclm_shared_apply (configs[4])
 */
#define GCLM_COMM_ID_BYTES 128
typedef struct gclm_comm gclm_comm;
int gclm_comm_unique_id(void* id_out /* GCLM_COMM_ID_BYTES */);
int gclm_comm_create(gclm_comm** out, const void* unique_id, int nranks, int rank, int device);
int gclm_comm_destroy(gclm_comm* c);
/* Message of the last failing call on this communicator; c == NULL: of the last failing gclm_comm_unique_id /
 * gclm_comm_create of the CALLING THREAD (thread-local, as gclm_last_error(NULL)). */
const char* gclm_comm_last_error(const gclm_comm* c);
/* NCCL_VERSION_CODE of the rccl.h this library was compiled against and ncclGetVersion() of the librccl it bound at
 * run time.  The library is not LINKED against librccl: on first use it takes the RCCL the process has already loaded
 * (a torch process: torch's own librccl.so, the one torch.distributed's communicators live in), otherwise
 * /opt/rocm/lib/librccl.so.1.  gclm_comm_create refuses (-21) a run-time library of another MAJOR version, and every
 * gclm_comm_* entry point fails with -22 when no librccl can be loaded at all (gclm_comm_last_error(NULL) then carries the
 * loader's message or the name of the missing entry point).  The choice is made by the first gclm_comm_unique_id /
 * gclm_comm_create of the process and holds for its lifetime: a process that also uses torch.distributed MUST import
 * torch before that call.  gclm_comm_versions itself never makes the choice: before one was made it reports the version
 * of the librccl already loaded in the process (what a binding now would pick), or runtime = 0 when none is loaded yet. */
int gclm_comm_versions(int* compiled, int* runtime);
int gclm_comm_all_gather(gclm_comm* c, const float* d_send, float* d_recv, size_t count_per_rank, void* stream);
int gclm_comm_all_reduce_sum(gclm_comm* c, float* d_buf, size_t count, void* stream);
int gclm_comm_all_reduce_sum_i32(gclm_comm* c, int32_t* d_buf, size_t count, void* stream);

/*
 * The reference's early stop is ONE decision over the whole batch (lm_optimizer.py:90-92, 619-625).  For a batch
 * sharded over the ranks of `c` (image sharding, configs[2]) that decision needs every rank's images: with a stop
 * communicator set, gclm_solve / gclm_calibrate sum the per-step counter of images whose cost still moved over the
 * ranks after every update (ONE 4-byte all-reduce per LM step, enqueued on the solve's stream, no host round trip), so
 * every rank stops at the step the single-process solve of the whole batch would stop at, and reports that `stop_at`.
 * Every rank must run the same num_steps.  NULL unsets it.  Without it a sharded solve must run with early_stop = 0.
 */
int gclm_set_stop_comm(gclm_handle* h, gclm_comm* c);

/* A batch of independent images solved as several PARTS by several handles (e.g. on several streams of one device, so
 * that one part's update launches run under another part's sweep; early_stop = 0): every output of a part is what the
 * single call would have produced for those images, except infos["stop_at"] -- the reference's "first step after which
 * EVERY image's cost was close" (lm_optimizer.py:619-620) is one number for the whole batch.  It re-derives stop_at from
 * the SUM of the parts' per-step counters and writes it into every row of every part's info.  At most 8 parts, same
 * device / num_steps.  The counters live in each handle's workspace and are those of the handle's LAST solve, so:
 *   - B[p] MUST be the batch size of part p's last gclm_solve / gclm_calibrate (checked: -2 otherwise); a part with
 *     B[p] == 0 is skipped (it holds no image: its handle need not have solved anything);
 *   - `stream` MUST be ordered after every part's solve (events / stream waits are the caller's business), and no part
 *     handle may start another solve before the merge kernel has run (it would overwrite the counters being summed). */
int gclm_merge_stop_at(gclm_handle* const* parts, float* const* d_info, const int* B, int n_parts, void* stream);

/* Tuning / test hook (no reference counterpart): loop iterations per workgroup of the sweep (how an image is cut
 * into partial records; only the summation order depends on it).  0 restores the built-in choice (20, fewer for
 * small batches).  Replaces the GCLM_SWEEP_ITERS environment variable of rounds 1-2: the solve reads no environment. */
int gclm_set_sweep_iters(gclm_handle* h, int iters);
/* How this handle's next solve of B images of (H, W) would cut an image into workgroup chunks: rows per chunk and
 * chunks per image (`aligned16`: all field pointers 16-byte aligned).  The cut fixes the summation order of an image's
 * partial records, so two calls agree bit for bit on an image exactly when their cuts agree; a caller that solves ONE
 * batch in several parts (gclm_merge_stop_at; LMOptimizer.overlap_streams) asks here instead of mirroring the rule.  The
 * cut depends on the batch size only below 2048 chunks per call (small batches take fewer rows per chunk to fill the
 * GPU).  Either output pointer may be NULL.  No device work, no error message: -1 for a NULL handle, -3 for a
 * non-positive B, H or W. */
int gclm_plan_cut(const gclm_handle* h, int B, int H, int W, int aligned16, int* rows_per_chunk, int* chunks_per_image);

/* sin(latitude_field) (lm_optimizer.py:262,270) does not depend on the parameters, yet each of the num_steps + 1 sweeps of
 * a solve would re-evaluate it per pixel.  For the VALU-bound distortion models the first sweep of a solve therefore
 * stores it in a LIBRARY-owned scratch plane (B x H x W floats inside the handle's workspace, grown on demand like the
 * rest of it) and every later sweep reads that plane instead of `latitude_field`: same bytes read per sweep, one extra
 * plane written per solve (1 / 105 of its traffic), same polynomial hence bit-identical results; the caller's boundary
 * (float32 radians) does not change.
 * mode -1 (default): the library decides (simple_radial / radial / simple_divisional with all five planes on the
 * 16-byte-aligned path, at least one LM step, not the one-launch-per-step path; never pinhole, which is memory-bound);
 * 0: never (saves B x H x W x 4 bytes of workspace); 1: wherever the sweep has the instantiation (also pinhole).
 *
 * The plane is OPTIONAL in every mode.  It is an allocation of its own, of exactly B x H x W x 4 bytes (no headroom; 1.26 GB
 * for 1024 images of 640x480, against 3 MB for the rest of the workspace), and a solve that cannot have it runs the sweeps
 * that compute sin(latitude) themselves -- the same bits, a few per cent slower -- instead of failing: when hipMalloc
 * fails, or when the plane would exceed the limit.  gclm_set_slat_plane_limit: max_bytes = 0 (default) = the built-in rule,
 * at most HALF of the device memory that is free when the plane is (re)allocated; otherwise a plane is only (re)allocated
 * while B x H x W x 4 <= max_bytes (1 = in effect never; a plane the handle already holds keeps serving the solves it is
 * large enough for -- gclm_release_workspace drops it; a larger plane replaces it only once that allocation has succeeded).  A
 * refused size is remembered until the limit or the mode is set again, or 64 further solves have wanted it,
 * so a serving loop does not pay a failing allocation per call.  Only the core workspace failing to allocate is an error
 * (-10).  A batch solved as n parts by n handles (LMOptimizer.overlap_streams) holds n planes of B / n images each: one
 * plane's worth in total.
 * A solve handed the caller's plane (gclm_solve_ex ...) where its sweeps read it needs no scratch plane, in every mode. */
int gclm_set_slat_plane(gclm_handle* h, int mode);
int gclm_set_slat_plane_limit(gclm_handle* h, size_t max_bytes);

/* Pinhole's batch sweep is bound by the bytes it reads: five float32 planes, 20 bytes per pixel, num_steps + 1 times.  The two
 * confidence planes compress for free: as 16-bit fixed point they move a solve by what float32 rounding inside it does (focal
 * 5e-7 relative, gravity 1e-7, final cost 5e-7 over 64 images of 48x64).  The first sweep of a pinhole solve can
 * therefore pack them into a LIBRARY-owned plane of one 32-bit word per pixel and every later sweep reads that plane in
 * their place: 16 bytes per pixel.  The caller's boundary (two float32 planes) does not change.  Format, on float32 values:
 *   q = rint(c * 65535) (round half to even), word = q_up | q_lat << 16, c' = float(q) * (1.0f / 65535.0f).
 * The first sweep evaluates every pixel with c' as well, so all sweeps of a solve see one objective, and a solve whose
 * confidences are already c' of some q returns the bits of the unpacked solve.
 * A confidence outside [0, 1], or a NaN, is never clamped: the first sweep evaluates that pixel with its own value and raises a
 * per-image flag on the device; every later sweep of a flagged image reads the caller's two planes (no host round trip).  Such
 * an image's first sweep uses c' for its in-range confidences and its later sweeps use c: a difference at the 1e-7 level.
 * mode -1 (default): the library decides (pinhole with all five planes on the 16-byte-aligned path, not the
 * one-launch-per-step path, no plane of sin(latitude) in use, at least 6 sweeps and B x H x W of at least 256 Mi pixels -- 874
 * images of 640x480; the plane pays from the smallest size measured, 32 Mi pixels, but below the threshold the sweeps' launch
 * time over the caller's five planes stays a true HBM rate, which the benchmark's records of such batches state); 0: never; 1: wherever the sweep has the instantiation (any batch size, 2 sweeps).
 * Sessions of gclm_shared_begin never pack.
 * The plane is B x H x W x 4 bytes, an optional allocation of its own under the rules of the sin(latitude) plane above
 * (gclm_set_slat_plane_limit governs both; a solve that cannot have it runs unpacked, never an error), refilled by every solve.
 * gclm_conf_pack_bytes: bytes of the plane the handle holds.  gclm_conf_pack_fallbacks: the number of flagged images of the
 * handle's last solve (0 if it did not pack) -- it SYNCHRONISES the device: for tests and diagnosis only. */
int gclm_set_conf_pack(gclm_handle* h, int mode);
/* *pack = would this handle's next solve of B images of (H, W) with `sweeps` sweeps (num_steps + 1) pack its confidences (1)
 * or not (0), memory permitting?  (`aligned16`: all field pointers 16-byte aligned; `five_planes`: a complete field set.)  For a caller that solves ONE batch in several parts and wants every part to take the
 * whole batch's decision (LMOptimizer.overlap_streams asks here and sets the parts' mode, instead of mirroring the rule).  No
 * device work, no error message: -1 for a NULL handle or pointer, -3 for a non-positive B, H or W. */
int gclm_plan_conf_pack(const gclm_handle* h, int B, int H, int W, int aligned16, int five_planes, int sweeps, int* pack);
size_t gclm_conf_pack_bytes(const gclm_handle* h);
int gclm_conf_pack_fallbacks(gclm_handle* h, int* n);

/* Row pairs (radial / simple_divisional).  Everything a radial camera model adds to the per-pixel work depends on
 * r2 = u^2 + v^2 only.  The principal point of every camera the library initialises is the image centre (camera.py:136-152),
 * so rows y and H - y of a column share r2 bit for bit; a lane of the sweep then takes row H - y along with row y and
 * evaluates the radial terms once for both (gclm_pass.hip: row_math_mirror; simple_divisional -14 % per sweep, radial -4 %).  The
 * per-pixel values are those of the one-row walk bit for bit; the order in which a lane adds its pixels differs, so results
 * agree with it to float32 summation order (~1e-7), not bit for bit.  An image whose principal point is NOT the centre
 * (an explicit camera handed to gclm_solve) is detected per image on the device and walks the same pairs without sharing.
 * mode -1 (default): the library decides (the models it pays for, all five planes on the 16-byte-aligned path, an even
 * number of rows, and more workgroups per launch than the one-launch-per-step path takes -- 768: below that a step is
 * latency-bound, and its two-launch form stays bit-identical to the one-launch form); 0: never (the one-row walk of every
 * earlier ABI, bit for bit); 1: wherever the sweep has the instantiation (also small launches, unless
 * gclm_set_fused_steps(h, 1) asks for one launch per step as well). */
int gclm_set_row_pairs(gclm_handle* h, int mode);

/* Small batches (the interactive single-image calibration of the reference's demo, interactive_demo.py:403) run ONE
 * launch per LM step: the per-image update of step k-1 is done in the prologue of every workgroup of sweep k
 * (num_steps + 2 launches per solve instead of 2 num_steps + 4 -- the first launch also builds the initial estimate; results
 * bit-identical to the two-launch sequence).
 * mode -1 (default): the library decides (few workgroups in flight); 0: never; 1: whenever it is valid (independent
 * intrinsics, 16-byte aligned fields of a width divisible by 4, and a single image or early_stop = 0 -- the
 * batch-global stop of lm_optimizer.py:619-625 is only decidable inside a launch when the batch is one image). */
int gclm_set_fused_steps(gclm_handle* h, int mode);

/* Single image with early_stop = 1 on the one-launch-per-step path: the launches after the stop return at their first
 * instruction, but each still takes its turn on the queue (21 of the 32 launches of a default-conf solve that stops at
 * step 9).  depth > 0 PACES the launches: launch k is issued once launch k - depth has reported to a word in
 * host-mapped memory, and none after the stop has been reported -- gclm_solve / gclm_calibrate then BLOCK the calling
 * thread for about the duration of the LM loop (the results are still produced asynchronously on the stream).  For
 * callers that read the result right away (the reference's GeoCalib.calibrate does: extractor.py:51-69).  0 (default)
 * = off: every launch is issued at once, the call returns immediately.  Ignored where it cannot help (more than one
 * image, early_stop = 0, the two-launch path).  Results do not depend on it.  depth in [0, 16]; 3 is a good value.
 * The host wait spins briefly, then yields between polls; if a report does not arrive within 2 ms (the queue is shared
 * with other streams) the rest of that solve is issued unpaced and the handle does not pace its next 64 solves. */
int gclm_set_paced_launches(gclm_handle* h, int depth);

/* Timing helper: when enabled, every sweep launch is bracketed by HIP events on the solve's stream;
 * gclm_last_pass_timing waits for the recorded launches, returns their count and summed duration
 * since the previous read, and resets the record.  Returns <0 if timing was not enabled. */
int gclm_set_timing(gclm_handle* h, int enabled);
int gclm_last_pass_timing(gclm_handle* h, int* n_launches, float* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* GCLM_H */
