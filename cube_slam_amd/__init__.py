"""cube_slam_amd -- MI355X-native kernels for CubeSLAM's per-frame hot path.

The compute lives in libcubeslam_hip.so (hand-written HIP for gfx950, C-ABI in include/cubeslam_hip.h); this
package is the thin host-side mirror of the reference interfaces used by tests and bench.py.
"""
from . import _lib  # noqa: F401
from .stereo import ComputeStereoMatches, StereoMatcher  # noqa: F401
from .rgbd import ClosePoints, ComputeStereoFromRGBD, RGBDAssociator  # noqa: F401
from .klt import KLTTracker, NewHarrisFeatures, SearchByTracking, SearchByTrackingHarris, calcOpticalFlowPyrLK, goodFeaturesToTrack  # noqa: F401
from .bow import KeyFrameDatabase, ORBVocabulary  # noqa: F401
from .local_mapping import ComputeDistinctiveDescriptors, KeyFrameView, LocalMapping, UpdateNormalAndDepth  # noqa: F401
from .initializer import Initializer  # noqa: F401
from .pnp_solver import PnPsolver  # noqa: F401
from .sim3_solver import Sim3Solver  # noqa: F401
from .tracking import Tracking  # noqa: F401
