"""Drop-in use from Python (MI355X): the two seams of the reference this package replaces.

    python examples/drop_in_python.py

(1) `GeoCalib.optimizer` (geocalib/geocalib.py:106,119): any code that calls `optimizer(data) -> dict` with the CNN's fields.
(2) `GeoCalib.calibrate(img, camera_model=..., priors=..., shared_intrinsics=...)` (geocalib/extractor.py:72-127) with a
    caller-supplied field network.
(3) `camera.undistort_image(image)` (geocalib/camera.py:396-412), which the reference's Gradio app calls right after calibrate().
    Its general form, `camera.upright_image(image, gravity)` and `camera.reproject_image(image, target, rotation)`, shows the
    image as another camera sees it: the horizon levelled with the estimated gravity, a wider pinhole camera (the interactive
    demo's padded undistortion), a clean image distorted, a virtual pan or tilt -- one gclm_reproject_image launch.

The CNN is out of scope of this package, so a stand-in "network" renders the perspective fields of a known camera
(gclm_synth_fields) at the resolution the reference's network would see; with the upstream package installed, pass its
model instead."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from geocalib_amd import GeoCalib, Gravity, LMOptimizer, camera_models, metrics  # noqa: E402
from geocalib_amd.synth import synth_fields  # noqa: E402

dev = torch.device("cuda:0")

# (1) the optimiser seam: fields in, camera / gravity / uncertainties out -- same conf keys, same dict keys as the reference
fields, gt_cam, gt_grav = synth_fields("simple_radial", 4, 480, 640, dev, seed=7)
opt = LMOptimizer({"camera_model": "simple_radial"}).eval()          # default conf: 30 steps, early stop on the device
out = opt(fields)
print("optimizer seam   : focal", [round(v, 1) for v in out["camera"].f[:, 1].tolist()], "(truth", [round(v, 1) for v in gt_cam[:, 3].tolist()], ")")
print("                   k1   ", [round(v, 4) for v in out["camera"].k1.tolist()], " stop_at", out["stop_at"].tolist())
print("                   roll / pitch [deg]", [tuple(round(x, 2) for x in rp) for rp in torch.rad2deg(out["gravity"].rp).tolist()])
print("                   focal_uncertainty", [round(v, 2) for v in out["focal_uncertainty"].tolist()])


# (2) the calibrate() front-end with a stand-in field network
def field_model(img_data):
    b, _, h, w = img_data["image"].shape
    f, _, _ = synth_fields("pinhole", b, h, w, img_data["image"].device, seed=3)
    return f


model = GeoCalib(field_model)                                     # paced_launches=3: calibrate() reads the camera right away
img = torch.rand(3, 768, 1024, device=dev)                        # any RGB image in [0, 1]
res = model.calibrate(img, camera_model="pinhole")
cam, grav = res["camera"], res["gravity"]
print("calibrate()      : image size", cam.size[0].tolist(), " focal", round(cam.f[0, 1].item(), 1), " vfov [deg]", round(torch.rad2deg(cam.vfov)[0].item(), 2))
print("                   roll / pitch [deg]", tuple(round(x, 2) for x in torch.rad2deg(grav.rp)[0].tolist()), " keys:", sorted(k for k in res if "uncertainty" in k))
res = model.calibrate(img, camera_model="pinhole", priors={"focal": torch.tensor(900.0, device=dev)})
print("with a focal prior: focal", round(res["camera"].f[0, 1].item(), 1))

# (3) remove the lens distortion: calibrate with a distortion model, then resample the image on the device
res = model.calibrate(img, camera_model="radial")
rect = res["camera"].undistort_image(img[None])                   # (1, 3, H, W): one gclm_undistort_image launch
print("undistort_image(): k1, k2", [round(v, 4) for v in res["camera"].dist[0].tolist()], " output", tuple(rect.shape))
level, seen = res["camera"].upright_image(img[None], res["gravity"], return_valid=True)       # undistorted and the roll removed
print("upright_image()  : output", tuple(level.shape), " pixels that see the source", round(seen.float().mean().item(), 3))

# (4) solve one batch from three starts -- the trivial and the heuristic initialisation, and the focal length held at a guess
#     (a prior) -- and keep, per image, the calibration that explains the fields best: one gclm_hypothesis_scores pass
starts = [LMOptimizer({"camera_model": "simple_radial", "init_conf": {"name": name}}).eval()(fields) for name in ("trivial", "heuristic")]
starts.append(opt({**fields, "prior_focal": torch.full((4,), 400.0, device=dev)}))
cams = camera_models["simple_radial"](torch.stack([s["camera"]._data for s in starts], 1))          # (B, N = 3)
gravs = Gravity(torch.stack([s["gravity"]._data for s in starts], 1))
ranked = metrics.rank_calibrations(fields, cams, gravs)              # inliers within 1 degree, weighted by the confidences
print("rank_calibrations(): best start per image", ranked["best"].tolist(), " scores", [[round(v) for v in r] for r in ranked["scores"].tolist()])
print("                   focal of the winners", [round(v, 1) for v in ranked["camera"].f[:, 1].tolist()])
