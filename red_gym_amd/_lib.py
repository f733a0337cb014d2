"""ctypes binding of include/f110_hip.h (libf110_hip.so, built by red_gym_amd.build).

There is no CPU fallback: if the HIP library is missing or fails to load the
import raises, and every entry point returning a negative code raises here.

The mirror is three literal tables -- SYMBOLS (+ RESTYPES), STRUCTS and the F110_* / E_* constants -- and
tests/test_abi_cpu.py checks them whole against the header: every prototype's return and argument types, every
struct's fields, sizes and offsets (by the C compiler), every constant.  An entry point is added to the header
and here; that test says where the two differ.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('F110_LIB') or os.path.join(_HERE, 'libf110_hip.so')  # F110_LIB: another build (tools/build_variant.sh)

F110_MAX_AGENTS = 32
F110_MAX_NOISE_SLOTS = 64
F110_MAX_MAPS = 4096
F110_NUM_PARAMS = 18
F110_RK4, F110_EULER = 1, 2
E_INVALID, E_HIP, E_NOMAP, E_INDEX, E_UNBOUND = -1, -2, -3, -4, -5

PARAM_KEYS = ['mu', 'C_Sf', 'C_Sr', 'lf', 'lr', 'h', 'm', 'I', 's_min', 's_max', 'sv_min', 'sv_max',
              'v_switch', 'a_max', 'v_min', 'v_max', 'width', 'length']


class Config(C.Structure):
    _fields_ = [('num_envs', C.c_int32), ('num_agents', C.c_int32), ('num_beams', C.c_int32),
                ('theta_dis', C.c_int32), ('integrator', C.c_int32), ('ego_idx', C.c_int32),
                ('device', C.c_int32), ('autoreset', C.c_int32), ('fov', C.c_double), ('eps', C.c_double),
                ('max_range', C.c_double), ('timestep', C.c_double), ('ttc_thresh', C.c_double),
                ('params', C.c_double * F110_NUM_PARAMS)]


BUFFER_FIELDS = ['state', 'steer_buf', 'steer_cnt', 'noise_step', 'spawn', 'start_rot', 'near_start',
                 'toggles', 'current_time', 'pending_reset', 'scans', 'scans_f64', 'pose_snap',
                 'collisions', 'collision_idx', 'in_collision', 'lap_counts', 'lap_times', 'done', 'checkpoint_done', 'lookups']


class BitmapConfig(C.Structure):
    _fields_ = [('device', C.c_int32), ('num_beams', C.c_int32), ('target_beam_count', C.c_int32),
                ('rows', C.c_int32), ('cols', C.c_int32), ('channels', C.c_int32), ('draw_mode', C.c_int32),
                ('bg_value', C.c_int32), ('draw_value', C.c_int32), ('draw_center', C.c_int32),
                ('scaling_factor', C.c_double)]


class Buffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in BUFFER_FIELDS]


# f110_progress_buffers: the progress tracker's caller-owned outputs, one element per car
PROGRESS_FIELDS = ['s', 'd', 'heading_error', 'delta', 'progress', 's_prev', 'seg', 'seen']


class ProgressBuffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in PROGRESS_FIELDS]


# f110_shaping_config / f110_shaping_buffers: the reward shaper's options and its caller-owned buffers
class ShapingConfig(C.Structure):
    _fields_ = [('rows', C.c_int32), ('cols', C.c_int32), ('agent', C.c_int32), ('neighborhood', C.c_int32),
                ('clip_max', C.c_int32), ('scale', C.c_double), ('origin_x', C.c_double), ('origin_y', C.c_double),
                ('max_lane_halfwidth', C.c_double), ('w_collision', C.c_double), ('w_progress', C.c_double),
                ('w_centering', C.c_double)]


SHAPING_FIELDS = ['bitmap', 'collision_term', 'progress_term', 'centering_term', 'total', 'collided', 'prev_xy', 't_seen', 'bitmap_bits']


class ShapingBuffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in SHAPING_FIELDS]


# f110_pathfollow_config / f110_pathfollow_buffers: the path follower's options and its caller-owned buffers
class PathFollowConfig(C.Structure):
    _fields_ = [('agent', C.c_int32), ('replan_at', C.c_int32), ('horizon', C.c_int32), ('reserved', C.c_int32),
                ('car_length', C.c_double), ('vector_length', C.c_double), ('max_diff_deg', C.c_double),
                ('dist_threshold', C.c_double), ('desired_velocity', C.c_double), ('timestep', C.c_double),
                ('q', C.c_double * 4), ('r', C.c_double * 2), ('p', C.c_double * 4), ('max_steer', C.c_double)]


PATHFOLLOW_FIELDS = ['path_points', 'path_index', 'path_replanned', 'mpc_accel', 't_seen']


class PathFollowBuffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in PATHFOLLOW_FIELDS]


# f110_replay_config / f110_replay_buffers: the replay buffer's options and its caller-owned ring
class ReplayConfig(C.Structure):
    _fields_ = [('steps', C.c_int32), ('action_dim', C.c_int32)]


REPLAY_FIELDS = ['frames', 'actions', 'rewards', 'dones', 'valid', 'count', 'chain_start', 't_seen', 'last_valid', 'action_in']
F110_REPLAY_TRIES = 64
F110_REPLAY_MAX_NSTEP = 64
F110_REPLAY_MAX_STACK = 8


class ReplayBuffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in REPLAY_FIELDS]


# f110_episodes_config / f110_episodes_buffers: the episode tracker's options and its caller-owned arrays
class EpisodesConfig(C.Structure):
    _fields_ = [('limit', C.c_int32), ('log', C.c_int32)]


EPISODES_FIELDS = ['ep_return', 'ep_length', 'ep_open', 't_seen', 'truncated', 'limit', 'log_env', 'log_length', 'log_return',
                   'log_reason', 'log_time', 'log_laps', 'count', 'block_counts']
F110_EPISODE_DONE, F110_EPISODE_LIMIT, F110_EPISODE_RESET = 1, 2, 3
F110_EPISODES_BLOCK = 256           # envs per entry of block_counts (the header's, which sizes the kernels' workgroups)


class EpisodesBuffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in EPISODES_FIELDS]


# f110_bitconv_config: the first convolution computed from bits (stateless)
class BitconvConfig(C.Structure):
    _fields_ = [('rows', C.c_int32), ('cols', C.c_int32), ('kernel', C.c_int32), ('stride', C.c_int32),
                ('channels', C.c_int32), ('relu', C.c_int32), ('on', C.c_float)]


F110_BITCONV_MAX_STACK = 8          # input channels of the stacked first convolution (f110_bitconv_forward_stack)


# f110_bitconv2_config: the policy stem (conv1 + relu + conv2) from bits, forward only (stateless)
class Bitconv2Config(C.Structure):
    _fields_ = [('rows', C.c_int32), ('cols', C.c_int32), ('kernel', C.c_int32), ('stride', C.c_int32),
                ('channels', C.c_int32), ('relu', C.c_int32), ('on', C.c_float),
                ('kernel2', C.c_int32), ('stride2', C.c_int32), ('channels2', C.c_int32), ('relu2', C.c_int32)]


# f110_featconv_config: a dense convolution of fp32 feature maps, forward and backward (stateless)
class FeatconvConfig(C.Structure):
    _fields_ = [('in_channels', C.c_int32), ('rows', C.c_int32), ('cols', C.c_int32), ('out_channels', C.c_int32),
                ('kernel', C.c_int32), ('stride', C.c_int32), ('relu', C.c_int32), ('reserved', C.c_int32)]


# f110_dense_config: a dense layer (fc1), forward and backward (stateless)
class DenseConfig(C.Structure):
    _fields_ = [('in_features', C.c_int32), ('out_features', C.c_int32), ('ld', C.c_int32), ('segment', C.c_int32),
                ('relu', C.c_int32), ('reserved', C.c_int32)]


# f110_policyhead_config: the policy head (fc_mean, fc_log_std and the sampling tail; stateless)
class PolicyheadConfig(C.Structure):
    _fields_ = [('in_features', C.c_int32), ('action_dim', C.c_int32), ('out_fp64', C.c_int32)]


F110_POLICYHEAD_SLICE_ROWS = 256


# f110_qhead_config, f110_qhead_critics, f110_qhead_grads: the critic head (the twin Q tail and the TD target; stateless)
class QheadConfig(C.Structure):
    _fields_ = [('hidden', C.c_int32), ('action_dim', C.c_int32), ('critics', C.c_int32), ('ld', C.c_int32), ('action_fp64', C.c_int32)]


QHEAD_CRITIC_FIELDS = ['pre', 'w_act', 'b1', 'w2', 'b2']
QHEAD_GRAD_FIELDS = ['grad_pre', 'grad_w_act', 'grad_b1', 'grad_w2', 'grad_b2']


class QheadCritics(C.Structure):
    _fields_ = [(name, C.c_void_p * 2) for name in QHEAD_CRITIC_FIELDS]


class QheadGrads(C.Structure):
    _fields_ = [(name, C.c_void_p * 2) for name in QHEAD_GRAD_FIELDS]


F110_QHEAD_SLICE_ROWS = 256


# f110_adam_config, f110_adam_tensor: the parameter update (Adam and the soft update of the targets); f110_adam_state lives on the device
class AdamConfig(C.Structure):
    _fields_ = [('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double), ('tau', C.c_double),
                ('with_target', C.c_int32), ('advance', C.c_int32)]


ADAM_TENSOR_FIELDS = ['p', 'g', 'm', 'v', 'target']


class AdamTensor(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ADAM_TENSOR_FIELDS] + [('n', C.c_int64)]


F110_ADAM_CHUNK = 4096
F110_ADAM_MAX_TENSORS = 64
F110_ADAM_STATE_BYTES = 32          # f110_adam_state: int64 t, double pow1, pow2, float k2, a
F110_ADAM_CLIP_STATE_BYTES = 64


# f110_adam_clip_state: the norm, the coefficient and the guard of a clipped step.  It lives on the device (a fresh one is zero bytes);
# a tagged typedef like the temperature's, mirrored here so that optim.py reads its offsets; tests/test_clip_cpu.py checks it against
# the compiler.
class AdamClipState(C.Structure):
    _fields_ = [('sumsq', C.c_double), ('norm', C.c_double), ('coef', C.c_float), ('skip', C.c_int32),
                ('steps_clipped', C.c_int64), ('steps_skipped', C.c_int64), ('reserved', C.c_int64 * 3)]


ADAM_CLIP_STRUCTS = {'f110_adam_clip_state': AdamClipState}


# f110_temperature_config, f110_temperature_state: the entropy temperature learnt on the device.  The state lives on the device and
# nests f110_adam_state by value; the mirror is here so that temperature.py writes a fresh state through it and reads its offsets.
class AdamState(C.Structure):
    _fields_ = [('t', C.c_int64), ('pow1', C.c_double), ('pow2', C.c_double), ('k2', C.c_float), ('a', C.c_float)]


class TemperatureConfig(C.Structure):
    _fields_ = [('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double), ('target_entropy', C.c_double)]


class TemperatureState(C.Structure):
    _fields_ = [('adam', AdamState), ('alpha', C.c_double), ('log_alpha', C.c_float), ('m', C.c_float), ('v', C.c_float),
                ('grad', C.c_float), ('loss', C.c_float), ('reserved', C.c_int32)]


# the header's tagged typedefs (a struct that nests another by value); tests/test_temperature_cpu.py checks them against the compiler
TEMPERATURE_STRUCTS = {'f110_adam_state': AdamState, 'f110_temperature_config': TemperatureConfig, 'f110_temperature_state': TemperatureState}

# f110_gauss_state: the policy's Gaussian draws.  The state lives on the device; the mirror is here so that gauss.py writes a fresh
# one through it and reads its offsets.  A tagged typedef like the temperature's; tests/test_gauss_cpu.py checks it against the compiler.
F110_GAUSS_STREAMS = 4
F110_GAUSS_MAX_COLUMNS = 32


class GaussState(C.Structure):
    _fields_ = [('seed', C.c_uint64), ('calls', C.c_uint64 * F110_GAUSS_STREAMS), ('reserved', C.c_uint64 * 3)]


GAUSS_STRUCTS = {'f110_gauss_state': GaussState}

# f110_priority_config, f110_priority_state, f110_priority_buffers: prioritized replay (tagged typedefs like the temperature's;
# tests/test_priority_cpu.py checks them against the compiler).  The state lives on the device: priority.py writes a fresh one through
# the mirror.
F110_PRIORITY_SHIFT = 16
F110_PRIORITY_MAX_LEAVES = 1 << 31
F110_PRIORITY_STATE_BYTES = 64


class PriorityConfig(C.Structure):
    _fields_ = [('exponent', C.c_double), ('eps', C.c_double)]


class PriorityState(C.Structure):
    _fields_ = [('qmax', C.c_uint32), ('reserved0', C.c_uint32), ('beta', C.c_double), ('beta_step', C.c_double), ('beta_end', C.c_double),
                ('reserved', C.c_uint64 * 4)]


class PriorityBuffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ('leaf', 'node', 'state')]


PRIORITY_STRUCTS = {'f110_priority_config': PriorityConfig, 'f110_priority_state': PriorityState, 'f110_priority_buffers': PriorityBuffers}

# every typedef struct of include/f110_hip.h but f110_adam_state (device-resident; F110_ADAM_STATE_BYTES is its size)
STRUCTS = {
    'f110_config': Config, 'f110_buffers': Buffers, 'f110_progress_buffers': ProgressBuffers,
    'f110_shaping_config': ShapingConfig, 'f110_shaping_buffers': ShapingBuffers,
    'f110_pathfollow_config': PathFollowConfig, 'f110_pathfollow_buffers': PathFollowBuffers,
    'f110_replay_config': ReplayConfig, 'f110_replay_buffers': ReplayBuffers,
    'f110_episodes_config': EpisodesConfig, 'f110_episodes_buffers': EpisodesBuffers,
    'f110_bitconv_config': BitconvConfig, 'f110_bitconv2_config': Bitconv2Config, 'f110_featconv_config': FeatconvConfig,
    'f110_dense_config': DenseConfig, 'f110_policyhead_config': PolicyheadConfig,
    'f110_qhead_config': QheadConfig, 'f110_qhead_critics': QheadCritics, 'f110_qhead_grads': QheadGrads,
    'f110_adam_config': AdamConfig, 'f110_adam_tensor': AdamTensor, 'f110_bitmap_config': BitmapConfig,
}

# every symbol include/f110_hip.h declares: name -> argtypes; RESTYPES below holds the return types that are not int
_VP, _I32, _I64, _D = C.c_void_p, C.c_int32, C.c_int64, C.c_double
SYMBOLS = {
    'f110_create': [C.POINTER(Config), C.POINTER(_VP)],
    'f110_destroy': [_VP],
    'f110_last_error': [],
    'f110_update_params': [_VP, _VP, _I32],
    'f110_set_tables': [_VP, _VP, _VP, _VP, _VP, _VP],
    'f110_set_map_occupancy': [_VP, _VP, _I32, _I32, _D, _D, _D, _D, _D],
    'f110_set_map_occupancy_dev': [_VP, _VP, _I32, _I32, _D, _D, _D, _D, _D],
    'f110_set_map_slot_occupancy': [_VP, _I32, _VP, _I32, _I32, _D, _D, _D, _D, _D],
    'f110_set_map_slot_occupancy_dev': [_VP, _I32, _VP, _I32, _I32, _D, _D, _D, _D, _D],
    'f110_assign_maps': [_VP, _VP],
    'f110_get_map_slot_dt': [_VP, _I32, _VP],
    'f110_track_mask': [_VP, _I32, _I32, _I32, _I32, _D, _D, _D, _D, _D, _VP, _VP],
    'f110_set_map_dt': [_VP, _VP, _I32, _I32, _D, _D, _D, _D, _D],
    'f110_get_map_dt': [_VP, _VP],
    'f110_edt_squared': [_VP, _I32, _I32, _VP],
    'f110_edt_squared_dev': [_VP, _I32, _I32, _VP, _VP],
    'f110_set_params_slots': [_VP, _VP, _I32],
    'f110_set_params_slot': [_VP, _I32, _VP, _I32],
    'f110_assign_params': [_VP, _VP],
    'f110_set_side_distance_slots': [_VP, _VP, _I32],
    'f110_set_noise_table': [_VP, _VP, _I64],
    'f110_set_noise_slot': [_VP, _I32, _VP, _I64],
    'f110_set_noise_generator': [_VP, _I32, _VP, _D],
    'f110_assign_noise': [_VP, _VP],
    'f110_set_noise_per_env': [_VP, _VP, _D],
    'f110_noise_ensure': [_VP, _I64, _VP],
    'f110_noise_prefetch': [_VP, _I64],
    'f110_noise_set_floor': [_VP, _I64, _VP],
    'f110_noise_info': [_VP, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)],
    'f110_noise_read': [_VP, _I32, _I64, _I64, _VP],
    'f110_device_errors': [_VP, C.POINTER(C.c_uint32)],
    'f110_bind': [_VP, C.POINTER(Buffers)],
    'f110_reset': [_VP, _VP, _VP, _VP],
    'f110_step': [_VP, _VP, _VP],
    'f110_pack_env_size': [_VP],
    'f110_pack_env': [_VP, _I32, _VP, _VP],
    'f110_set_scan_stages': [_VP, C.c_char_p],
    'f110_launch_epoch': [_VP, C.POINTER(C.c_int64)],
    'f110_set_scan_order': [_VP, _VP],
    'f110_scan_form_info': [_VP, _I32, C.POINTER(C.c_int32), C.POINTER(C.c_double)],
    'f110_scan_form_learn': [_VP, _VP, _VP],
    'f110_scan_rows_info': [_VP, _I32, C.POINTER(C.c_int32)],
    'f110_scan_codes_info': [_VP, _I32, C.POINTER(C.c_int32)],
    'f110_scan_pad_rows': [_VP, C.POINTER(C.c_int32)],
    'f110_graph_create': [_VP, _VP, _I32, C.POINTER(_VP)],
    'f110_graph_launch': [_VP, _VP],
    'f110_graph_info': [_VP, C.POINTER(C.c_int32), C.c_char_p],
    'f110_graph_destroy': [_VP],
    'f110_pure_pursuit': [_VP, _VP, _I32, _D, _D, _D, _D, _VP, _I32, _VP, _VP],
    'f110_pure_pursuit_prepare': [_VP, _VP, _I32, _D, _D, _VP],
    'f110_pure_pursuit_workspace': [_I32, _I32],
    'f110_pure_pursuit_tracks': [_VP, _VP, _VP, _VP, _I32, _VP, _D, _D, _D, _D, _VP, _I32, _VP, _VP, _I32, _VP],
    'f110_progress_validate': [_VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _I32],
    'f110_progress_install': [_VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _I32],
    'f110_progress_bind': [_VP, C.POINTER(ProgressBuffers)],
    'f110_progress_update': [_VP, _VP],
    'f110_shaping_validate': [C.POINTER(ShapingConfig), _I32],
    'f110_shaping_install': [_VP, C.POINTER(ShapingConfig)],
    'f110_shaping_bind': [_VP, C.POINTER(ShapingBuffers)],
    'f110_shaping_update': [_VP, _VP],
    'f110_shaping_terms': [C.POINTER(ShapingConfig), _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_shaping_terms_bits': [C.POINTER(ShapingConfig), _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_pathfollow_validate': [C.POINTER(PathFollowConfig), _I32],
    'f110_pathfollow_install': [_VP, C.POINTER(PathFollowConfig)],
    'f110_pathfollow_bind': [_VP, C.POINTER(PathFollowBuffers)],
    'f110_pathfollow_act': [_VP, _VP, _VP, _VP],
    'f110_pathfollow_update': [_VP, _VP],
    'f110_pathfollow_decode': [C.POINTER(PathFollowConfig), _VP, _VP, _I32, _VP, _VP],
    'f110_pathfollow_mpc': [C.POINTER(PathFollowConfig), _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_pathfollow_advance': [C.POINTER(PathFollowConfig), _VP, _VP, _VP, _I32, _VP, _VP],
    'f110_replay_validate': [C.POINTER(ReplayConfig), C.POINTER(ShapingConfig), _I32],
    'f110_replay_install': [_VP, C.POINTER(ReplayConfig)],
    'f110_replay_bind': [_VP, C.POINTER(ReplayBuffers)],
    'f110_replay_update': [_VP, _VP],
    'f110_replay_draw': [_VP, C.c_uint64, C.c_uint64, _I32, _VP, _VP, _VP],
    'f110_replay_gather': [_VP, _VP, _I32, _VP, _VP, _I32, _D, _VP, _VP, _VP, _VP, _VP],
    'f110_replay_locate': [_VP, _VP, _I32, _VP, _VP, _VP],
    'f110_replay_sample': [_VP, C.c_uint64, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_replay_nstep': [_VP, _VP, _I32, _I32, _D, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_replay_sample_nstep': [_VP, C.c_uint64, _VP, _I32, _I32, _D, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_replay_stack': [_VP, _VP, _I32, _I32, _VP, _VP, _VP],
    'f110_priority_node_words': [_I64],
    'f110_ptree_rebuild': [_VP, _VP, _I64, _VP],
    'f110_ptree_set': [_VP, _VP, _I64, _VP, _VP, _I32, _VP],
    'f110_ptree_pick': [_VP, _VP, _I64, C.c_uint64, C.c_uint64, _I32, _VP, _VP, _VP],
    'f110_priority_install': [_VP, _VP],
    'f110_priority_bind': [_VP, _VP],
    'f110_priority_reset': [_VP, _VP],
    'f110_priority_sample': [_VP, C.c_uint64, _VP, _I32, _I32, _D, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_priority_update': [_VP, _VP, _VP, _VP, _I32, _VP, _VP],
    'f110_priority_set': [_VP, _VP, _VP, _I32, _VP],
    'f110_episodes_validate': [C.POINTER(EpisodesConfig)],
    'f110_episodes_install': [_VP, C.POINTER(EpisodesConfig)],
    'f110_episodes_bind': [_VP, C.POINTER(EpisodesBuffers)],
    'f110_episodes_update': [_VP, _VP],
    'f110_episodes_apply': [C.POINTER(EpisodesConfig), _I32, _D, _VP, _VP, _VP, _VP, _I64, _VP, C.POINTER(EpisodesBuffers), _VP],
    'f110_bitconv_validate': [C.POINTER(BitconvConfig)],
    'f110_bitconv_workspace': [C.POINTER(BitconvConfig), _I64],
    'f110_bitconv_forward': [C.POINTER(BitconvConfig), _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP],
    'f110_bitconv_forward_u8': [C.POINTER(BitconvConfig), _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP],
    'f110_bitconv_backward': [C.POINTER(BitconvConfig), _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _VP],
    'f110_bitconv_forward_stack': [C.POINTER(BitconvConfig), _VP, _I64, _VP, _I32, _I64, _VP, _VP, _VP, _VP],
    'f110_bitconv_workspace_stack': [C.POINTER(BitconvConfig), _I32, _I64],
    'f110_bitconv_backward_stack': [C.POINTER(BitconvConfig), _VP, _I64, _VP, _I32, _I64, _VP, _VP, _VP, _VP, _VP],
    'f110_bitconv2_validate': [C.POINTER(Bitconv2Config)],
    'f110_bitconv2_forward': [C.POINTER(Bitconv2Config), _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_bitconv2_forward_u8': [C.POINTER(Bitconv2Config), _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_bitconv2_forward_stack': [C.POINTER(Bitconv2Config), _VP, _I64, _VP, _I32, _I64, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_featconv_validate': [C.POINTER(FeatconvConfig)],
    'f110_featconv_workspace': [C.POINTER(FeatconvConfig), _I64],
    'f110_featconv_forward': [C.POINTER(FeatconvConfig), _VP, _I64, _VP, _VP, _VP, _VP],
    'f110_featconv_backward': [C.POINTER(FeatconvConfig), _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_dense_validate': [C.POINTER(DenseConfig)],
    'f110_dense_workspace': [C.POINTER(DenseConfig), _I64],
    'f110_dense_forward': [C.POINTER(DenseConfig), _VP, _I64, _VP, _VP, _VP, _VP, _VP],
    'f110_dense_backward': [C.POINTER(DenseConfig), _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP],
    'f110_policyhead_validate': [C.POINTER(PolicyheadConfig)],
    'f110_policyhead_workspace': [C.POINTER(PolicyheadConfig), _I64],
    'f110_policyhead_forward': [C.POINTER(PolicyheadConfig), _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_policyhead_backward': [C.POINTER(PolicyheadConfig), _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_qhead_validate': [C.POINTER(QheadConfig)],
    'f110_qhead_workspace': [C.POINTER(QheadConfig), _I64],
    'f110_qhead_forward': [C.POINTER(QheadConfig), C.POINTER(QheadCritics), _VP, _I64, _VP, _VP, _VP, _D, _D, _VP, _VP, _VP, _VP],
    'f110_qhead_backward': [C.POINTER(QheadConfig), C.POINTER(QheadCritics), _VP, _I64, _VP, _VP, _VP, C.POINTER(QheadGrads), _VP, _VP, _VP],
    'f110_adam_validate': [C.POINTER(AdamConfig)],
    'f110_adam_state_bytes': [],
    'f110_adam_step': [C.POINTER(AdamConfig), C.POINTER(AdamTensor), _I32, _VP, _D, _VP],
    'f110_soft_update': [C.POINTER(AdamTensor), _I32, _D, _VP],
    'f110_adam_clip_state_bytes': [],
    'f110_adam_gradnorm': [C.POINTER(AdamTensor), _I32, _I64, _VP, _I64, _VP],
    'f110_adam_clip': [_VP, _I64, _D, _VP, _VP],
    'f110_adam_step_clipped': [C.POINTER(AdamConfig), C.POINTER(AdamTensor), _I32, _VP, _VP, _D, _VP],
    'f110_sac_critic_loss': [_VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP],
    'f110_sac_actor_loss': [_VP, _I32, _VP, _D, _I64, _VP, _VP, _VP, _VP],
    'f110_sac_critic_loss_weighted': [_VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP],
    'f110_temperature_validate': [_VP],
    'f110_temperature_state_bytes': [],
    'f110_temperature_step': [_VP, _VP, _I32, _I64, _VP, _D, _VP],
    'f110_qhead_forward_alpha_dev': [C.POINTER(QheadConfig), C.POINTER(QheadCritics), _VP, _I64, _VP, _VP, _VP, _D, _VP, _VP, _VP, _VP, _VP],
    'f110_sac_actor_loss_alpha_dev': [_VP, _I32, _VP, _VP, _I64, _VP, _VP, _VP, _VP],
    'f110_qhead_forward_rows': [C.POINTER(QheadConfig), C.POINTER(QheadCritics), _VP, _I64, _VP, _VP, _VP, _VP, _D, _VP, _VP, _VP, _VP, _VP],
    'f110_gauss_state_bytes': [],
    'f110_gauss_fill': [_VP, _I32, _I64, _I32, _VP, _VP, _I32, _VP],
    'f110_gauss_fill_at': [C.c_uint64, _I32, C.c_uint64, _I64, _I32, _VP, _VP, _VP],
    'f110_replay_pack': [_VP, _I64, _I32, _I32, _VP, _VP],
    'f110_replay_unpack': [_VP, _I64, _I32, _I32, _VP, _VP],
    'f110_profile_begin': [_VP, _I32],
    'f110_profile_every': [_VP, _I32],
    'f110_profile_end': [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int32)],
    'f110_scan': [_VP, _VP, _I32, _VP, _VP, _VP, _VP],
    'f110_update_pose': [_VP, _VP, _VP, _VP, _VP, _I32, _VP],
    'f110_vehicle_dynamics': [_VP, _VP, _VP, _I32, _I32, _VP, _VP],
    'f110_get_vertices': [_VP, _VP, _I32, _VP, _VP],
    'f110_gjk_pairs': [_VP, _VP, _VP, _I32, _VP, _VP],
    'f110_collision_multiple': [_VP, _VP, _I32, _I32, _VP, _VP, _VP],
    'f110_check_ttc': [_VP, _VP, _VP, _I32, _VP, _VP],
    'f110_check_ttc_slots': [_VP, _VP, _VP, _VP, _I32, _VP, _VP],
    'f110_ray_cast': [_VP, _VP, _VP, _I32, _VP, _VP, _VP],
    'f110_check_done': [_VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    'f110_bitmap_create': [C.POINTER(BitmapConfig), _VP, _VP, _VP, C.POINTER(_VP)],
    'f110_bitmap_destroy': [_VP],
    'f110_bitmap_render': [_VP, _VP, _I32, _I64, _I64, _VP, _VP],
    'f110_bitmap_render_bits': [_VP, _VP, _I32, _I64, _I64, _VP, _VP],
    'f110_bitmap_points': [_VP, _VP, _I32, _I64, _I64, _VP, _VP],
    'f110_scan_occupancy': [_VP, _I32, _I64, _I64, _I32, _VP, _VP, _D, _D, _D, _I32, _VP, _VP],
}
RESTYPES = {
    'f110_last_error': C.c_char_p,
    'f110_destroy': None, 'f110_graph_destroy': None, 'f110_bitmap_destroy': None,
    'f110_pack_env_size': _I64, 'f110_adam_state_bytes': _I64, 'f110_adam_clip_state_bytes': _I64, 'f110_temperature_state_bytes': _I64,
    'f110_gauss_state_bytes': _I64, 'f110_priority_node_words': _I64,
    'f110_pure_pursuit_workspace': _I64, 'f110_bitconv_workspace': _I64, 'f110_bitconv_workspace_stack': _I64, 'f110_featconv_workspace': _I64,
    'f110_dense_workspace': _I64, 'f110_policyhead_workspace': _I64, 'f110_qhead_workspace': _I64,
}


class F110Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('f110 error %d: %s' % (code, msg))
        self.code = code


_lib = None


def load():
    """Loads libf110_hip.so; raises if it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError('%s not found: build it with `python -m red_gym_amd.build` '
                          '(hipcc --offload-arch=gfx950); there is no CPU fallback.' % LIB_PATH)
    # torch bundles its own libamdhip64 (soname libamdhip64.so.7).  It must be in the
    # process BEFORE this library is loaded so that both share ONE HIP runtime (ours then
    # binds to the already-loaded soname); the other order maps a second runtime, which
    # cannot see the device.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
        fn.argtypes = argtypes
        fn.restype = RESTYPES.get(name, C.c_int)
    _lib = lib
    return lib


def clamp(v):
    """int(v) clamped into int32: an out-of-range size reaches the library's validate, which can name it."""
    return max(min(int(v), 2 ** 31 - 1), -2 ** 31)


def ptr(t):
    """data_ptr() of a tensor, NULL for None."""
    return None if t is None else t.data_ptr()


def stream(dev):
    """The raw handle of the caller's current stream on `dev`."""
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def check(rc):
    """Maps C error codes to the exceptions the reference raises for the same
    conditions (ValueError base_classes.py:619 / laser_models.py:446, IndexError :527)."""
    if rc == 0:
        return
    msg = load().f110_last_error().decode('utf-8', 'replace')
    if rc in (E_INVALID, E_NOMAP):
        raise ValueError(msg)
    if rc == E_INDEX:
        raise IndexError(msg)
    raise F110Error(rc, msg)
