"""ctypes binding of ``libsbc_hip.so`` (C ABI declared in ``include/sbc_hip.h``).

There is no fallback: if the shared library is missing or a call fails, an exception is raised -- the
product path never routes around the HIP kernels.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SBC_LIB_PATH') or os.path.join(_HERE, 'libsbc_hip.so')   # env override: A/B builds (tools/)
ABI_VERSION = 16

EXPORTS = ('sbc_abi_version', 'sbc_set_persistent_cus', 'sbc_last_error', 'sbc_device_count', 'sbc_op_launch', 'sbc_plan_create',
           'sbc_plan_run', 'sbc_plan_set_persistent_cus', 'sbc_plan_destroy', 'sbc_plan_profile', 'sbc_plan_profile_read',
           'sbc_pack_conv_weight', 'sbc_pack_conv_weight_winograd',
           'sbc_pack_conv_weight_split', 'sbc_pack_conv_weight_winograd_split',
           'sbc_pack_conv_weight_f16', 'sbc_pack_conv_weight_winograd_f16',
           'sbc_pack_conv_weight_f16x2', 'sbc_pack_conv_weight_winograd_f16x2', 'sbc_pack_conv_weight_pooled_f16x2', 'sbc_range_flag',
           'sbc_f16x2_calibration_input', 'sbc_f16x2_calibrate', 'sbc_debug_philox4x32', 'sbc_debug_complex_normal',
           'sbc_score_create', 'sbc_score_buffers', 'sbc_score_ops', 'sbc_score_level_source', 'sbc_score_forward',
           'sbc_score_destroy', 'sbc_score_wiring_create', 'sbc_score_wiring_read', 'sbc_score_wiring_destroy', 'sbc_score_wiring_bind', 'sbc_wgrad_scratch_floats', 'sbc_l1_lifted_run', 'sbc_ls_regularized',
           'sbc_em_gm_amp_run',
           'sbc_ldamp_create', 'sbc_ldamp_destroy', 'sbc_ldamp_workspace_floats', 'sbc_ldamp_denoise', 'sbc_ldamp_run', 'sbc_ldamp_stage',
           'sbc_ldamp_trainer_create', 'sbc_ldamp_trainer_destroy', 'sbc_ldamp_trainer_workspace_floats', 'sbc_ldamp_trainer_step',
           'sbc_ldamp_trainer_adam', 'sbc_ldamp_trainer_stage', 'sbc_ldamp_trainer_get_state', 'sbc_ldamp_trainer_set_state',
           'sbc_debug_ldamp_directions',
           'sbc_wgan_create', 'sbc_wgan_destroy', 'sbc_wgan_workspace_floats', 'sbc_wgan_generate', 'sbc_wgan_run', 'sbc_wgan_stage',
           'sbc_wgan_trainer_create', 'sbc_wgan_trainer_destroy', 'sbc_wgan_trainer_workspace_floats', 'sbc_wgan_trainer_critic_step',
           'sbc_wgan_trainer_generator_step', 'sbc_wgan_trainer_stage', 'sbc_wgan_trainer_copy', 'sbc_wgan_wgrad128_scratch_floats',
           'sbc_wgan_wgrad128', 'sbc_wgan_bn_backward', 'sbc_wgan_rmsprop',
           'sbc_link_code_create', 'sbc_link_code_destroy', 'sbc_link_encode', 'sbc_link_llr', 'sbc_link_decode', 'sbc_link_errors',
           'sbc_link_simulate')


class SbcError(RuntimeError):
    pass


class sbc_op(C.Structure):
    _fields_ = [('kind', C.c_int32), ('flags', C.c_int32),
                ('B', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('cin', C.c_int32), ('cout', C.c_int32), ('ksize', C.c_int32), ('dil', C.c_int32),
                ('up_h', C.c_int32), ('up_w', C.c_int32), ('tag', C.c_int32),
                ('in_', C.c_void_p), ('out', C.c_void_p), ('weight', C.c_void_p), ('bias', C.c_void_p),
                ('stats', C.c_void_p), ('res1', C.c_void_p), ('res2', C.c_void_p), ('up', C.c_void_p),
                ('ext', C.c_void_p), ('weight_wino', C.c_void_p), ('weight_split', C.c_void_p),
                ('weight_wino_split', C.c_void_p),
                # training operators (ABI 7)
                ('grad', C.c_void_p), ('aux', C.c_void_p), ('wgrad', C.c_void_p), ('bgrad', C.c_void_p),
                ('weight2_split', C.c_void_p),
                ('calib', C.c_void_p),                # ABI 11: NULL (set by sbc_f16x2_calibrate on its own copies)
                ('bias2', C.c_void_p), ('norm2', C.c_void_p),   # ABI 12: RES_BLOCK (second convolution's bias, second norm's alpha|gamma|beta)
                ('weight2_wino_split', C.c_void_p),             # ABI 13: calibration only (every form of a layer gets the same scale)
                # ABI 14: launch lanes of a plan (0 = the run stream), event ids recorded behind / waited for in front of the record
                ('lane', C.c_int32), ('signal', C.c_int32), ('wait', C.c_int32 * 2)]


class sbc_endconv(C.Structure):
    _fields_ = [('sigmas', C.c_void_p), ('labels', C.c_void_p), ('sigma_of_step', C.c_void_p),
                ('step', C.c_void_p)]


class sbc_langevin(C.Structure):
    _fields_ = [('X', C.c_void_p), ('score', C.c_void_p), ('P', C.c_void_p), ('p_index', C.c_void_p),
                ('Y', C.c_void_p), ('Htrue', C.c_void_p), ('h_index', C.c_void_p), ('sched', C.c_void_p),
                ('group', C.c_void_p), ('noise', C.c_void_p), ('nmse', C.c_void_p), ('step', C.c_void_p),
                ('traj_id', C.c_void_p), ('meas_scale', C.c_void_p), ('seed', C.c_uint64),
                ('n_steps', C.c_int32), ('Nt', C.c_int32), ('Nr', C.c_int32), ('Np', C.c_int32)]


class sbc_dsm(C.Structure):
    _fields_ = [('sigmas', C.c_void_p), ('labels', C.c_void_p), ('noise', C.c_void_p), ('sample_id', C.c_void_p),
                ('seed', C.c_uint64), ('offset', C.c_int32), ('anneal_power', C.c_float), ('step', C.c_void_p),
                ('grad_scale', C.c_float)]


class sbc_adam(C.Structure):
    _fields_ = [('n', C.c_int64), ('lr', C.c_double), ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double),
                ('ema_mu', C.c_double), ('step', C.c_void_p)]


class sbc_chain(C.Structure):
    _fields_ = [('n_blocks', C.c_int32), ('type', C.c_int32 * 6), ('dil', C.c_int32 * 6), ('w1', C.c_void_p * 6), ('w2', C.c_void_p * 6),
                ('w1_wino', C.c_void_p * 6), ('w2_wino', C.c_void_p * 6), ('w3', C.c_void_p * 6), ('bias1', C.c_void_p * 6),
                ('bias2', C.c_void_p * 6), ('bias3', C.c_void_p * 6), ('norm1', C.c_void_p * 6), ('norm2', C.c_void_p * 6)]


class sbc_tensor_ref(C.Structure):
    _fields_ = [('name', C.c_char_p), ('data', C.c_void_p), ('numel', C.c_int64)]


class sbc_score_desc(C.Structure):
    _fields_ = [('ngf', C.c_int32), ('channels', C.c_int32), ('nt', C.c_int32), ('nr', C.c_int32), ('batch', C.c_int32),
                ('conv_mode', C.c_int32), ('sigmas', C.c_void_p), ('num_classes', C.c_int32), ('flags', C.c_int32)]


# the wiring of the score network (plan.py reads it; ABI 15)
class sbc_skip_branch(C.Structure):
    _fields_ = [('branch', C.c_char_p), ('anchor', C.c_char_p), ('lane', C.c_int32)]


class sbc_score_wiring_desc(C.Structure):
    _fields_ = [('ngf', C.c_int32), ('channels', C.c_int32), ('nt', C.c_int32), ('nr', C.c_int32), ('flags', C.c_int32),
                ('pair_shapes', C.POINTER(C.c_int32)), ('n_pair_shapes', C.c_int32), ('skip', C.POINTER(sbc_skip_branch)), ('n_skip', C.c_int32),
                ('conv_mode', C.c_int32)]             # ABI 16: -1 = no gates, or CONV_MODE_IDS[...]


class sbc_wiring_tensor(C.Structure):
    _fields_ = [('name', C.c_char_p), ('h', C.c_int32), ('w', C.c_int32), ('c', C.c_int32), ('slot', C.c_int32)]


class sbc_wiring_block(C.Structure):
    _fields_ = [('type', C.c_int32), ('dil', C.c_int32)] + [(k, C.c_char_p) for k in ('w1', 'w2', 'bias1', 'bias2', 'norm1', 'norm2', 'w3', 'bias3')]


class sbc_wiring_record(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ('kind', 'flags', 'ksize', 'dil', 'tag', 'src', 'dst', 'stats', 'res1', 'res2', 'up', 'moments', 'geom',
                                         'side', 'join', 'lane', 'signal')] + \
               [('wait', C.c_int32 * 2), ('first_block', C.c_int32), ('n_blocks', C.c_int32)] + \
               [(k, C.c_char_p) for k in ('name', 'weight', 'bias', 'weight2', 'bias2', 'norm2', 'norm_key')]


class sbc_score_wiring_view(C.Structure):
    _fields_ = [('tensors', C.POINTER(sbc_wiring_tensor)), ('records', C.POINTER(sbc_wiring_record)), ('blocks', C.POINTER(sbc_wiring_block)),
                ('slot_elems', C.POINTER(C.c_int64))] + [(k, C.c_int32) for k in ('n_tensors', 'n_records', 'n_blocks', 'n_slots', 'x', 'out', 'n_chains')]


# sbc_score_wiring_bind (scorenet.py; ABI 16)
CONV_MODE_IDS = {'bf16x3': 0, 'f32': 1, 'f16w': 2, 'f16x2': 3}      # sbc_score_desc / sbc_score_wiring_desc / sbc_score_bind_desc .conv_mode


class sbc_named_ptr(C.Structure):
    _fields_ = [('name', C.c_char_p), ('ptr', C.c_void_p)]


class sbc_score_bind_desc(C.Structure):
    _fields_ = [('batch', C.c_int32), ('conv_mode', C.c_int32), ('slots', C.POINTER(C.c_void_p)), ('n_slots', C.c_int32),
                ('params', C.POINTER(sbc_named_ptr)), ('n_params', C.c_int32), ('endconv', C.POINTER(sbc_endconv))]


# classical baselines (baselines.py): lifted-DFT l1 (Lasso / fsAD) and regularised least squares (ML)
class sbc_l1_lifted_desc(C.Structure):
    _fields_ = [('P', C.c_void_p), ('p_index', C.c_void_p), ('Y', C.c_void_p), ('Htrue', C.c_void_p), ('h_index', C.c_void_p),
                ('lmbda', C.c_void_p), ('lr', C.c_void_p), ('nmse', C.c_void_p), ('H_hat', C.c_void_p), ('X', C.c_void_p),
                ('B', C.c_int32), ('nP', C.c_int32), ('nH', C.c_int32), ('Nt', C.c_int32), ('Nr', C.c_int32), ('Np', C.c_int32),
                ('lifting', C.c_int32), ('steps', C.c_int32)]


class sbc_ls_desc(C.Structure):
    _fields_ = [('P', C.c_void_p), ('p_index', C.c_void_p), ('Y', C.c_void_p), ('noise_var', C.c_void_p), ('Htrue', C.c_void_p),
                ('h_index', C.c_void_p), ('H_hat', C.c_void_p), ('nmse', C.c_void_p),
                ('B', C.c_int32), ('nP', C.c_int32), ('nH', C.c_int32), ('Nt', C.c_int32), ('Nr', C.c_int32), ('Np', C.c_int32)]


# EM-GM-AMP (baselines.em_gm_amp)
class sbc_em_gm_amp_desc(C.Structure):
    _fields_ = [('P', C.c_void_p), ('p_index', C.c_void_p), ('Y', C.c_void_p), ('Htrue', C.c_void_p), ('h_index', C.c_void_p),
                ('nmse', C.c_void_p), ('H_hat', C.c_void_p), ('X', C.c_void_p), ('params', C.c_void_p), ('stop_iter', C.c_void_p),
                ('B', C.c_int32), ('nP', C.c_int32), ('nH', C.c_int32), ('Nt', C.c_int32), ('Nr', C.c_int32), ('Np', C.c_int32),
                ('nit', C.c_int32), ('em_iters', C.c_int32), ('theta', C.c_float), ('tol', C.c_float)]


# Learned D-AMP (ldamp.py)
class sbc_ldamp_run_desc(C.Structure):
    _fields_ = [('Y_herm', C.c_void_p), ('P_herm', C.c_void_p), ('eig1', C.c_void_p), ('directions', C.c_void_p), ('Htrue', C.c_void_p),
                ('H_hat', C.c_void_p), ('nmse', C.c_void_p), ('h_log', C.c_void_p), ('z_log', C.c_void_p), ('div_log', C.c_void_p),
                ('eps_log', C.c_void_p), ('workspace', C.c_void_p), ('seed', C.c_uint64), ('sample0', C.c_int64),
                ('B', C.c_int32), ('Np', C.c_int32), ('Nt', C.c_int32), ('Nr', C.c_int32), ('num_unrolls', C.c_int32)]


# Learned D-AMP training (ldamp.Trainer)
class sbc_ldamp_step_desc(C.Structure):
    _fields_ = [('Y_herm', C.c_void_p), ('P_herm', C.c_void_p), ('eig1', C.c_void_p), ('directions', C.c_void_p), ('Htrue', C.c_void_p),
                ('loss', C.c_void_p), ('h_log', C.c_void_p), ('z_log', C.c_void_p), ('div_log', C.c_void_p), ('eps_log', C.c_void_p),
                ('workspace', C.c_void_p), ('seed', C.c_uint64), ('sample0', C.c_int64), ('lr', C.c_double), ('step', C.c_int64),
                ('B', C.c_int32), ('Np', C.c_int32), ('Nt', C.c_int32), ('Nr', C.c_int32), ('num_unrolls', C.c_int32)]


# WGAN latent optimisation (wgan.py)
class sbc_wgan_run_desc(C.Structure):
    _fields_ = [('Y', C.c_void_p), ('P', C.c_void_p), ('H', C.c_void_p), ('z', C.c_void_p), ('m', C.c_void_p), ('v', C.c_void_p),
                ('lr', C.c_void_p), ('l2_lam', C.c_void_p), ('loss_scale', C.c_void_p), ('oracle_log', C.c_void_p),
                ('meas_log', C.c_void_p), ('reg_log', C.c_void_p), ('z_log', C.c_void_p), ('g_log', C.c_void_p), ('workspace', C.c_void_p),
                ('B', C.c_int32), ('Np', C.c_int32), ('first_step', C.c_int32), ('n_steps', C.c_int32)]


# WGAN training (wgan.Trainer)
class sbc_wgan_trainer_desc(C.Structure):
    _fields_ = [('lr_d', C.c_double), ('lr_g', C.c_double), ('alpha', C.c_double), ('eps', C.c_double), ('clamp_lower', C.c_double),
                ('clamp_upper', C.c_double)]


# coded link simulation (link.py)
LINK_DEVICE_RANDOM, LINK_NO_CLIP = 1, 2


class sbc_link_code_desc(C.Structure):
    _fields_ = [('base', C.c_void_p), ('interleaver', C.c_void_p), ('rows', C.c_int32), ('cols', C.c_int32), ('Z', C.c_int32)]


class sbc_link_random(C.Structure):
    _fields_ = [('seed', C.c_uint64), ('packet0', C.c_int64), ('snr_index', C.c_int32), ('flags', C.c_int32)]


class sbc_link_encode_desc(C.Structure):
    _fields_ = [('payload', C.c_void_p), ('codeword', C.c_void_p), ('symbols', C.c_void_p), ('Npk', C.c_int32), ('S', C.c_int32),
                ('rnd', sbc_link_random)]


class sbc_link_llr_desc(C.Structure):
    _fields_ = [('symbols', C.c_void_p), ('Hp_ideal', C.c_void_p), ('Hp_est', C.c_void_p), ('chan_index', C.c_void_p), ('noise', C.c_void_p),
                ('llr_ideal', C.c_void_p), ('llr_est', C.c_void_p), ('noise_power', C.c_float), ('Npk', C.c_int32), ('pool', C.c_int32),
                ('Nr', C.c_int32), ('S', C.c_int32), ('rnd', sbc_link_random)]


class sbc_link_sim_desc(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ('Hp_ideal', 'Hp_est', 'payload', 'chan_index', 'noise', 'ber_ideal', 'bler_ideal', 'ber_est',
                                          'bler_est', 'iters_ideal', 'iters_est')] + \
               [('noise_power', C.c_float), ('Npk', C.c_int32), ('pool', C.c_int32), ('Nr', C.c_int32), ('S', C.c_int32),
                ('max_iters', C.c_int32), ('rnd', sbc_link_random)]


_lib = None


def lib():
    """Load the library once; raise ``SbcError`` with a build hint if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SbcError('%s not found: build it with `make -C %s` (or `python -c "import __graft_entry__ as g; '
                       'g.build()"`); there is no CPU fallback' % (LIB_PATH, os.path.join(_HERE, 'csrc')))
    h = C.CDLL(LIB_PATH)
    h.sbc_abi_version.restype = C.c_int
    h.sbc_last_error.restype = C.c_char_p
    h.sbc_device_count.restype = C.c_int
    h.sbc_op_launch.argtypes = [C.POINTER(sbc_op), C.c_void_p]
    h.sbc_plan_create.argtypes = [C.POINTER(sbc_op), C.c_int32, C.POINTER(C.c_void_p)]
    h.sbc_plan_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    h.sbc_plan_set_persistent_cus.argtypes = [C.c_void_p, C.c_int32]
    h.sbc_plan_destroy.argtypes = [C.c_void_p]
    h.sbc_plan_destroy.restype = None
    h.sbc_plan_profile.argtypes = [C.c_void_p, C.c_int32]
    h.sbc_plan_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    h.sbc_pack_conv_weight.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    h.sbc_pack_conv_weight_winograd.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    h.sbc_pack_conv_weight_split.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    h.sbc_pack_conv_weight_winograd_split.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    h.sbc_pack_conv_weight_f16.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    h.sbc_pack_conv_weight_winograd_f16.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    h.sbc_pack_conv_weight_f16x2.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    h.sbc_pack_conv_weight_winograd_f16x2.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    h.sbc_pack_conv_weight_pooled_f16x2.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    h.sbc_range_flag.argtypes = [C.POINTER(C.c_int32), C.c_int32]
    h.sbc_f16x2_calibration_input.argtypes = [C.c_void_p, C.c_int64]
    h.sbc_f16x2_calibrate.argtypes = [C.POINTER(sbc_op), C.c_int32, C.c_void_p]
    h.sbc_debug_philox4x32.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    h.sbc_debug_complex_normal.argtypes = [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]
    h.sbc_score_create.argtypes = [C.POINTER(sbc_score_desc), C.POINTER(sbc_tensor_ref), C.c_int32, C.POINTER(C.c_void_p)]
    h.sbc_score_buffers.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    h.sbc_score_ops.argtypes = [C.c_void_p, C.POINTER(C.POINTER(sbc_op)), C.POINTER(C.c_int32)]
    h.sbc_score_level_source.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    h.sbc_score_forward.argtypes = [C.c_void_p, C.c_void_p]
    h.sbc_score_destroy.argtypes = [C.c_void_p]
    h.sbc_score_destroy.restype = None
    h.sbc_score_wiring_create.argtypes = [C.POINTER(sbc_score_wiring_desc), C.POINTER(C.c_void_p)]
    h.sbc_score_wiring_read.argtypes = [C.c_void_p, C.POINTER(sbc_score_wiring_view)]
    h.sbc_score_wiring_destroy.argtypes = [C.c_void_p]
    h.sbc_score_wiring_destroy.restype = None
    h.sbc_score_wiring_bind.argtypes = [C.c_void_p, C.POINTER(sbc_score_bind_desc), C.POINTER(sbc_op), C.POINTER(sbc_chain)]
    h.sbc_wgrad_scratch_floats.argtypes = [C.c_int32] * 6
    h.sbc_wgrad_scratch_floats.restype = C.c_int64
    h.sbc_l1_lifted_run.argtypes = [C.POINTER(sbc_l1_lifted_desc), C.c_void_p]
    h.sbc_ls_regularized.argtypes = [C.POINTER(sbc_ls_desc), C.c_void_p]
    h.sbc_em_gm_amp_run.argtypes = [C.POINTER(sbc_em_gm_amp_desc), C.c_void_p]
    h.sbc_ldamp_create.argtypes = [C.POINTER(sbc_tensor_ref), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    h.sbc_ldamp_destroy.argtypes = [C.c_void_p]
    h.sbc_ldamp_destroy.restype = None
    h.sbc_ldamp_workspace_floats.argtypes = [C.c_int32, C.c_int32]
    h.sbc_ldamp_workspace_floats.restype = C.c_int64
    h.sbc_ldamp_denoise.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    h.sbc_ldamp_run.argtypes = [C.c_void_p, C.POINTER(sbc_ldamp_run_desc), C.c_void_p]
    h.sbc_ldamp_stage.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    h.sbc_debug_ldamp_directions.argtypes = [C.c_uint64, C.c_int64, C.c_int32, C.c_void_p]
    h.sbc_ldamp_trainer_create.argtypes = [C.POINTER(sbc_tensor_ref), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    h.sbc_ldamp_trainer_destroy.argtypes = [C.c_void_p]
    h.sbc_ldamp_trainer_destroy.restype = None
    h.sbc_ldamp_trainer_workspace_floats.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    h.sbc_ldamp_trainer_workspace_floats.restype = C.c_int64
    h.sbc_ldamp_trainer_step.argtypes = [C.c_void_p, C.POINTER(sbc_ldamp_step_desc), C.c_void_p]
    h.sbc_ldamp_trainer_adam.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int64, C.c_void_p]
    h.sbc_ldamp_trainer_stage.argtypes = [C.c_int32] * 5 + [C.POINTER(C.c_int64)] + [C.POINTER(C.c_int32)] * 4
    h.sbc_ldamp_trainer_get_state.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int64)]
    h.sbc_ldamp_trainer_set_state.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    h.sbc_wgan_create.argtypes = [C.POINTER(sbc_tensor_ref), C.c_int32, C.POINTER(C.c_void_p)]
    h.sbc_wgan_destroy.argtypes = [C.c_void_p]
    h.sbc_wgan_destroy.restype = None
    h.sbc_wgan_workspace_floats.argtypes = [C.c_void_p, C.c_int32]
    h.sbc_wgan_workspace_floats.restype = C.c_int64
    h.sbc_wgan_generate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    h.sbc_wgan_run.argtypes = [C.c_void_p, C.POINTER(sbc_wgan_run_desc), C.c_void_p]
    h.sbc_wgan_stage.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32)]
    h.sbc_wgan_trainer_create.argtypes = [C.POINTER(sbc_wgan_trainer_desc), C.POINTER(sbc_tensor_ref), C.c_int32, C.POINTER(sbc_tensor_ref), C.c_int32,
                                          C.POINTER(C.c_void_p)]
    h.sbc_wgan_trainer_destroy.argtypes = [C.c_void_p]
    h.sbc_wgan_trainer_destroy.restype = None
    h.sbc_wgan_trainer_workspace_floats.argtypes = [C.c_void_p, C.c_int32]
    h.sbc_wgan_trainer_workspace_floats.restype = C.c_int64
    h.sbc_wgan_trainer_critic_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    h.sbc_wgan_trainer_generator_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    h.sbc_wgan_trainer_stage.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64)] + [C.POINTER(C.c_int32)] * 4
    h.sbc_wgan_trainer_copy.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_void_p, C.c_int64, C.c_int32]
    h.sbc_wgan_wgrad128_scratch_floats.argtypes = [C.c_int32] * 4
    h.sbc_wgan_wgrad128_scratch_floats.restype = C.c_int64
    h.sbc_wgan_wgrad128.argtypes = [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.c_void_p]
    h.sbc_wgan_bn_backward.argtypes = [C.c_void_p] * 6 + [C.c_float] + [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p]
    h.sbc_wgan_rmsprop.argtypes = [C.c_void_p] * 3 + [C.c_int64] + [C.c_double] * 5 + [C.c_int32, C.c_void_p]
    h.sbc_link_code_create.argtypes = [C.POINTER(sbc_link_code_desc), C.POINTER(C.c_void_p)]
    h.sbc_link_code_destroy.argtypes = [C.c_void_p]
    h.sbc_link_code_destroy.restype = None
    h.sbc_link_encode.argtypes = [C.c_void_p, C.POINTER(sbc_link_encode_desc), C.c_void_p]
    h.sbc_link_llr.argtypes = [C.c_void_p, C.POINTER(sbc_link_llr_desc), C.c_void_p]
    h.sbc_link_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    h.sbc_link_errors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    h.sbc_link_simulate.argtypes = [C.c_void_p, C.POINTER(sbc_link_sim_desc), C.c_void_p]
    if h.sbc_abi_version() != ABI_VERSION:
        raise SbcError('libsbc_hip.so ABI %d != expected %d' % (h.sbc_abi_version(), ABI_VERSION))
    _lib = h
    return h


def check(rc):
    if rc != 0:
        raise SbcError('libsbc_hip: %s (status %d)' % (lib().sbc_last_error().decode(), rc))


def check_against_spec(sd, spec):
    """Raise ``KeyError`` / ``ValueError`` like ``load_state_dict(strict=True)`` would; ``spec``: ordered ``[(name, shape)]``."""
    import numpy as np
    names = dict(spec)
    missing = [n for n, _ in spec if n not in sd]
    unexpected = [n for n in sd if n not in names]
    if missing or unexpected:
        raise KeyError('state_dict mismatch: missing %s, unexpected %s' % (missing[:5], unexpected[:5]))
    for n, shape in spec:
        if tuple(np.shape(sd[n])) != tuple(shape):
            raise ValueError('size mismatch for %s: %s vs %s' % (n, tuple(np.shape(sd[n])), tuple(shape)))


def tensor_refs(sd, names):
    """``(sbc_tensor_ref[len(names)], keepalive)`` over ``sd[name]`` as contiguous float32 host arrays.  The refs hold bare pointers:
    ``keepalive`` must outlive the call they are passed to."""
    import numpy as np
    names = list(names)
    keep = [np.ascontiguousarray(sd[n], dtype=np.float32) for n in names]
    enc = [n.encode() for n in names]
    refs = (sbc_tensor_ref * len(names))(*[sbc_tensor_ref(enc[i], a.ctypes.data_as(C.c_void_p), a.size) for i, a in enumerate(keep)])
    return refs, (keep, enc)


class DeviceHandle:
    """Base of the classes that own one library handle with its weights on a torch device (``ldamp.LDAMP``,
    ``wgan.DCGAN_G_Ours``): device resolution, the grow-only workspace tensor and the handle's lifetime.  A subclass names the
    library function that frees its handle in ``_destroy``."""
    _destroy = None

    def __init__(self, device=None):
        self.device = device
        self._h = None
        self._ws = None
        self.last_workspace = None                       # (tensor, n_images) of the last call, for stage()

    def cuda(self, device=None):
        self.device = device if device is not None else self.device
        return self

    def eval(self):
        return self

    def _torch_device(self):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError('%s needs a HIP device (there is no CPU fallback)' % type(self).__name__)
        d = self.device
        if d is None:
            return torch.device('cuda', torch.cuda.current_device())
        d = torch.device(d)
        return d if d.index is not None else torch.device('cuda', torch.cuda.current_device())

    def _need_weights(self):
        if self._h is None:
            raise RuntimeError('%s has no weights: call load_state_dict first' % type(self).__name__)

    def _load(self, sd, names, create):
        """Replace the handle by the one ``create(refs, len(names), byref(handle))`` makes of ``sd``'s tensors ``names`` on this
        object's device; the old handle is freed only once the new one exists."""
        import torch
        refs, keep = tensor_refs(sd, names)              # (keep: the host arrays, alive until create has copied them)
        handle = C.c_void_p()
        with torch.cuda.device(self._torch_device()):
            check(create(refs, len(refs), C.byref(handle)))
        self.close()
        self._h = handle
        return self

    def _workspace_of(self, n, dev):
        """The workspace tensor, re-allocated only when ``n`` floats do not fit or the device changed."""
        import torch
        if self._ws is None or self._ws.numel() < n or self._ws.device != dev:
            self._ws = None                              # (released before its replacement is allocated)
            self._ws = torch.empty(max(int(n), 1), dtype=torch.float32, device=dev)
        return self._ws

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def numpy_state_dict(state):
    """A ``state_dict`` of torch tensors and / or array-likes as ``{name: numpy array}`` on the host."""
    import numpy as np
    return {k: (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)) for k, v in state.items()}


RANGE_OVERFLOW, RANGE_UNDERFLOW, RANGE_ELU = 1, 2, 4


def range_flag(reset=True, device=None):
    """``sbc_range_flag`` of ``device`` (default: the current one): the bit set the f16x2 convolutions collected since the last
    reset -- ``RANGE_OVERFLOW``: a staged activation left the fp16 range; ``RANGE_UNDERFLOW``: a region of an input was so far
    below its layer's calibrated scale that the two-term split there is no longer fp32-class.  Waits for every stream of the
    device."""
    v = C.c_int32()
    if device is not None:
        import torch
        with torch.cuda.device(device):
            check(lib().sbc_range_flag(C.byref(v), 1 if reset else 0))
    else:
        check(lib().sbc_range_flag(C.byref(v), 1 if reset else 0))
    return v.value


def describe_range(bits):
    what = []
    if bits & RANGE_OVERFLOW:
        what.append('an activation left the fp16 range (|x| * act_scale >= 16000)')
    if bits & RANGE_UNDERFLOW:
        what.append('a region of an input stayed below 2^-6 of its layer\'s scale (denormal low terms)')
    if bits & RANGE_ELU:
        what.append('a fused RCU launch met inputs below 2^-4, where its exp(x) - 1 form of ELU loses relative accuracy')
    return '; '.join(what)


def check_range(what='run', device=None):
    """Raise if the f16x2 kernels flagged this run: its numbers are not fp32-class (``driver.run_trajectories`` re-runs such a
    batch in ``bf16x3`` instead of raising)."""
    bits = range_flag(True, device)
    if bits:
        raise SbcError('%s: %s in conv_mode f16x2; results are not fp32-class -- use conv_mode bf16x3 for this input'
                       % (what, describe_range(bits)))


def calibration_input(n):
    """The library's fixed calibration pattern (``sbc_f16x2_calibration_input``) as a float32 numpy array of ``n`` values."""
    import numpy as np
    x = np.empty(int(n), np.float32)
    check(lib().sbc_f16x2_calibration_input(x.ctypes.data_as(C.c_void_p), int(n)))
    return x


def calibrate_f16x2(ops, stream):
    """``sbc_f16x2_calibrate`` over a list of bound ``sbc_op`` records (synchronises ``stream``)."""
    arr = (sbc_op * len(ops))(*ops)
    check(lib().sbc_f16x2_calibrate(arr, len(ops), C.c_void_p(stream)))


class Plan:
    """Owner of an ``sbc_plan*``.  ``keepalive`` holds whatever owns the device buffers the ops point to."""

    def __init__(self, ops, keepalive=None):
        arr = (sbc_op * len(ops))(*ops)
        handle = C.c_void_p()
        check(lib().sbc_plan_create(arr, len(ops), C.byref(handle)))
        self._h = handle
        self._keep = keepalive
        self.n_ops = len(ops)

    def run(self, stream, n_iters=1, use_graph=False):
        # use_graph: False / True (a flat graph: lane records in list order on the run stream) / 2 (lanes as parallel branches of the graph)
        check(lib().sbc_plan_run(self._h, C.c_void_p(stream), int(n_iters), 2 if use_graph == 2 else 1 if use_graph else 0))

    def set_persistent_cus(self, n):
        """Grid width (CUs) of this plan's persistent kernels; 0 = the process default (``sbc_plan_set_persistent_cus``)."""
        check(lib().sbc_plan_set_persistent_cus(self._h, int(n)))

    def profile(self, tag):
        check(lib().sbc_plan_profile(self._h, int(tag)))

    def profile_read(self):
        ms, n = C.c_double(), C.c_int64()
        check(lib().sbc_plan_profile_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def close(self):
        if self._h:
            lib().sbc_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
