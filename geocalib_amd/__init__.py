"""geocalib_amd -- MI355X-native (gfx950) implementation of GeoCalib's LM calibration path.

Public surface (mirrors the reference's geocalib package for this path):
    LMOptimizer                         geocalib/lm_optimizer.py:141   (+ optimizer_step, update_lambda, early_stop; conf
                                        "differentiable": gradients through the LM steps to the fields and confidences,
                                        .loss / .metrics of siclib/models/optimization/lm_optimizer.py:577-625)
    lm_grad                             the recorded HIP solve, its HIP adjoint, and lm_unrolled_torch: the unrolled loop in torch
    Camera models / camera_models       geocalib/camera.py
    Gravity                             geocalib/gravity.py
    GeoCalib (extractor with calibrate) geocalib/extractor.py:15  (CNN supplied by the caller)
    metrics                             siclib/models/utils/metrics.py  (+ perspective_field_metrics: fields against a calibration,
                                        rank_calibrations: N candidate calibrations per image against its fields)
    RPFSolver, solve_rpf                siclib/models/optimization/ransac.py  (the three-pixel minimal solver and RANSAC over it)
    viz                                 geocalib/interactive_demo.py: render_frame  (draw_perspective_fields: the fields drawn over an image)
    perspective_encoding                siclib/models/utils/perspective_encoding.py  (fields as classification bins; with
                                        fields.pack_fields_from_logits: classification heads to fields in one pass)
    PerspectiveParamOpt                 siclib/models/optimization/perspective_opt.py  (Adam on roll, pitch, vfov against the
                                        fields, batched; perspective_opt.cost_function: its cost and gradient in one pass)
    losses                              siclib/models/decoders/{up,latitude,perspective}_decoder.py: calculate_losses, loss
                                        (perspective_field_loss: the heads' training losses against a calibration,
                                        differentiable in the predicted fields, one HIP pass each way;
                                        perspective_bin_loss: the classification heads' cross-entropy against a calibration's
                                        bins, differentiable in the logits, one HIP pass each way)
    pack_fields                         geocalib/geocalib.py:57,73-75  (fields.pack_fields: the heads' epilogue in one HIP pass,
                                        float32 / float16 / bfloat16 raws; with a raw that requires grad the outputs carry a
                                        graph and backward is one more pass -- raw head outputs -> fields -> {losses, LM})
"""
from .camera import BaseCamera, Pinhole, Radial, SimpleDivisional, SimpleRadial, camera_models  # noqa: F401
from .gravity import Gravity  # noqa: F401
from .lm_optimizer import LMOptimizer, get_trivial_estimation  # noqa: F401
from .extractor import GeoCalib  # noqa: F401,E402
from . import metrics  # noqa: F401,E402
from .ransac import RPFSolver, solve_rpf  # noqa: F401,E402
from . import viz  # noqa: F401,E402
from . import perspective_encoding  # noqa: F401,E402
from .perspective_opt import PerspectiveParamOpt  # noqa: F401,E402
from . import losses  # noqa: F401,E402
from .losses import perspective_bin_loss, perspective_decoder_loss, perspective_field_loss  # noqa: F401,E402
from . import lm_grad  # noqa: F401,E402
from .fields import pack_fields  # noqa: F401,E402

__version__ = "0.1.0"
