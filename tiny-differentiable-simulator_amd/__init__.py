"""tiny-differentiable-simulator_amd — MI355X-native many-instance replay of the TDS
per-environment step.  Import through the repo-root alias ``tds_amd`` (the directory name
is not a valid Python identifier)."""
from .model import *  # noqa: F401,F403
from . import model  # noqa: F401

from . import hip_backend  # noqa: F401,E402
from .hip_backend import params_apply  # noqa: F401,E402
from . import ranks  # noqa: F401,E402
from . import vec_env  # noqa: F401,E402
from .vec_env import VectorizedAntEnv, VectorizedLaikagoEnv, VectorizedEnv  # noqa: F401,E402
from .autograd import step_fn, param_step_fn, rb_rollout_fn, trajectory_fn, policy_trajectory_fn, contact_fn  # noqa: F401,E402
from .autograd import dynamics_fn, inverse_dynamics_fn  # noqa: F401,E402
from .ilqr import ilqr, QuadraticCost  # noqa: F401,E402
from .sysid import sysid, sysid_starts  # noqa: F401,E402
