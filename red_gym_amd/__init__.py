"""MI355X-native batched F1TENTH environment (the F110Env.step hot path of
WE-Autopilot/red_gym as hand-written HIP kernels behind a C ABI).

    from red_gym_amd import F110VecEnv, F110Env, Integrator
"""
from .base_classes import Integrator  # noqa: F401


def __getattr__(name):
    # heavy imports (torch) only when the env classes are actually requested
    if name in ('F110VecEnv', 'VecObs'):
        from . import vec_env
        return getattr(vec_env, name)
    if name == 'F110Env':
        from .f110_env import F110Env
        return F110Env
    if name in ('lidar_to_bitmap', 'LidarBitmap', 'scan_occupancy'):
        from . import lidar
        return getattr(lidar, name)
    if name in ('conv_bits', 'BitConv2d', 'conv_bits2', 'BitConvStem'):
        from . import bitconv
        return getattr(bitconv, name)
    if name in ('conv_feat', 'FeatConv2d', 'Trunk'):
        from . import featconv
        return getattr(featconv, name)
    if name in ('linear_feat', 'Dense'):
        from . import dense
        return getattr(dense, name)
    if name in ('sample_actions', 'PolicyHead'):
        from . import policyhead
        return getattr(policyhead, name)
    if name in ('twin_q', 'td_target', 'QHead'):
        from . import qhead
        return getattr(qhead, name)
    if name in ('SacAdam', 'soft_update'):
        from . import optim
        return getattr(optim, name)
    if name in ('critic_loss', 'actor_loss'):
        from . import sacloss
        return getattr(sacloss, name)
    if name == 'Temperature':
        from .temperature import Temperature
        return Temperature
    if name == 'GaussianSource':
        from .gauss import GaussianSource
        return GaussianSource
    if name in ('EpisodeTracker', 'DONE', 'LIMIT', 'RESET'):
        from . import episodes
        return getattr(episodes, name)
    if name == 'SACAgent':
        from .sac import SACAgent
        return SACAgent
    raise AttributeError(name)
