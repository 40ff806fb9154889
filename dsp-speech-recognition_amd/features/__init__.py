"""MI355X-native drop-in for the reference's ``features`` package (DSP feature front-end).

Put ``dsp-speech-recognition_amd/`` on ``sys.path`` ahead of the reference checkout and
``from features import mfcc, delta, to_frames`` / ``from features.endpoint import
basic_endpoint_detection`` (model.py:2,13) resolve here.  Same function names, arguments, defaults
and return types as features/{sigproc,base,endpoint,preprocess}.py; the arithmetic runs in
hand-written HIP kernels (gfx950) behind a ctypes C ABI (include/dsp_frontend.h).

Unlike the reference's ``features/__init__.py`` this import has no side effects (no ./log/
directory, no matplotlib / sklearn import).  Both pitch trackers (``pitch_detect_sr``, ``pitch_detect``) and
``pitch_feature`` are here, and ``features.ensemble`` evaluates the fitted pitch SVM and the ensemble's confidence gate
(pitch_model.py:54-61, ensemble.py:44-67) on the device; ``features.svmfit`` fits that scaler and SVM there as well
(pitch_model.py:26-50: ``fit_pitch_svm``, ``grid_search``, ``PitchModelTrainer``).
``get_batch_full(feat)`` is RNNModel.get_batch_full (model.py:114-135) for the reference's list of (sig, rate) pairs, the
rates mixed as reader.mini_batch_iterator yields them.  ``TrainBatch`` is the training step of model.py:137-147 on raw clips
with the lengths kept on the device (features/train.py), and ``DeviceAdam`` its optimiser step (model.py:140-149) with the
state on the device, recordable behind the backward (features/optim.py).  ``MixedRateCapacityBatch`` and ``MixedRateTrainBatch``
serve mixed-rate batches of any lengths and rate assignments through one recorded launch sequence: the grouping by rate is device work.
``DeviceRng`` and ``device_dropout`` (features/dropout.py) draw the heads' dropouts from a counter-based generator on the device:
the heads' ``rng=`` keyword makes an eager step and a graph replay draw the same multipliers.
``Metrics`` and ``cross_entropy`` (features/metrics.py) keep the loss, its gradient, the accuracy, the confusion matrix and the
list of wrong clips on the device, and ``Trainer`` (features/fit.py) is model.py's ``train`` mode with one download per epoch.
There is no CPU fallback: without the built library or without a GPU every compute call raises.
"""
from .base import *  # noqa: F401,F403
from .sigproc import *  # noqa: F401,F403
from .endpoint import *  # noqa: F401,F403
from .preprocess import *  # noqa: F401,F403
from .pitch import (center_clip, max_pitch, pitch_detect_frame_sr, pitch_detect_sr,  # noqa: F401
                    robust_max_pitch, smooth, window, pitch_detect, pitch_detect_frame, peak_score,
                    sub_endpoint_detect, find_smooth_subsequence, slope, quad_params, peakshift, pitch_feature,
                    pitch_feature_batch, pitch_features_device)
from . import base, sigproc, endpoint, preprocess, pitch, batch, pipeline, ensemble, train, optim, svmfit, dropout, metrics, fit  # noqa: F401
from .batch import FeaturePlan, EndpointPlan  # noqa: F401
from .pipeline import VadMfccPipeline  # noqa: F401
from .ensemble import PitchSVM, EnsembleBatch, MixedRateEnsembleBatch, ensemble_decide  # noqa: F401
from .model_glue import MixedRateFeatureBatch, MixedRateCapacityBatch, get_batch_full  # noqa: F401
from .svmfit import fit_pitch_svm, grid_search, robust_scale_fit, svm_fit_problems, PitchModelTrainer  # noqa: F401
from .train import TrainBatch, MixedRateTrainBatch, AdvTrainBatch  # noqa: F401
from .optim import DeviceAdam  # noqa: F401
from .dropout import DeviceRng, device_dropout  # noqa: F401
from .metrics import Metrics, cross_entropy  # noqa: F401
from .fit import Trainer  # noqa: F401
