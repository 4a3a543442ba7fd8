"""megapose6d_amd -- MI355X-native render-and-compare pose engine behind the megapose6d inference API.

Only what the hot path needs: the HIP/C-ABI engine (`csrc/`, `_lib`, `engine`) and the host-side mirror
of the reference's renderer / PosePredictor / PoseEstimator interfaces.  Importing the package never touches the GPU; the
first engine call loads `libmp_engine.so` and raises if it is missing (there is no CPU fallback).
"""
from . import (detector, distances, distributed, engine, evaluation, icp_refiner, load_model, mask_rcnn, mesh_cleanup, mesh_db, mesh_io, object_dataset, onboarding, pose_estimator,  # noqa: F401
               pose_rigid, prediction_runner, renderer, scene_renderer, symmetries, tcoll, template_detector, types, visualization)
from .detector import Detector  # noqa: F401
from .icp_refiner import DepthRefiner, ICPRefiner, TeaserppRefiner  # noqa: F401
from .mask_rcnn import DetectorMaskRCNN  # noqa: F401
from .object_dataset import RigidObject, RigidObjectDataset  # noqa: F401
from .onboarding import (TsdfVolume, reconstruct_object, reconstruct_object_unposed, track_views, volume_for_first_view,  # noqa: F401
                         volume_for_views)
from .load_model import NAMED_MODELS, create_model_pose, load_named_model, load_pose_models  # noqa: F401
from .pose_estimator import CoarseRefinePoseEstimator, PoseEstimator  # noqa: F401
from .pose_rigid import PosePredictor  # noqa: F401
from .prediction_runner import PredictionRunner  # noqa: F401
from .renderer import Panda3dBatchRenderer  # noqa: F401
from .scene_renderer import Panda3dSceneRenderer  # noqa: F401
from .template_detector import TemplateMatchingModel, TemplateSet, make_template_detector, select_features  # noqa: F401
from .symmetries import ContinuousSymmetry, DiscreteSymmetry, make_symmetries_poses  # noqa: F401
from .types import (BatchRenderOutput, CameraRenderingData, ObservationTensor, Panda3dCameraData, Panda3dLightData,  # noqa: F401
                    Panda3dObjectData, PosePredictorOutput)

__version__ = "0.1.0"
