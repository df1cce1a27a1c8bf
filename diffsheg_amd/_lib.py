"""ctypes binding of libdiffsheg_hip.so (include/diffsheg_hip.h).

There is deliberately no fallback: if the HIP library is missing the import of any product module
fails with a clear message (build it with ``python -c 'import __graft_entry__ as g; g.build()'`` or
``make -C diffsheg_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdiffsheg_hip.so")


class DshError(RuntimeError):
    pass


class ModelConfigC(C.Structure):
    _fields_ = [("dim_pose", C.c_int32), ("expression_dim", C.c_int32), ("style_dim", C.c_int32),
                ("classifier_free", C.c_int32), ("cond_scale", C.c_float), ("latent_dim", C.c_int32),
                ("ff_size", C.c_int32), ("num_layers", C.c_int32), ("num_heads", C.c_int32),
                ("audio_dim", C.c_int32), ("aud_latent_dim", C.c_int32), ("hubert_dim", C.c_int32),
                ("hubert_enc_dim", C.c_int32), ("precision", C.c_int32), ("single_transformer", C.c_int32),
                ("diffusion_steps", C.c_int32)]        # (0: 1000)


class CrossAttnWeightsC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("norm_g", "norm_b", "text_norm_g", "text_norm_b", "wq", "bq", "wk", "bk", "wv", "bv",
                                           "sty_norm_g", "sty_norm_b", "sty_emb_w", "sty_emb_b", "sty_out_w", "sty_out_b")]


class SamplerOptsC(C.Structure):
    _fields_ = [("kind", C.c_int32), ("diffusion_steps", C.c_int32), ("respacing", C.c_int32),
                ("jump_length", C.c_int32), ("jump_n_sample", C.c_int32), ("overlap_len", C.c_int32),
                ("add_blend", C.c_int32), ("no_resample", C.c_int32), ("no_repaint", C.c_int32),
                ("clip_denoised", C.c_int32), ("noise_mode", C.c_int32), ("seed", C.c_uint64),
                ("same_overlap_noisy", C.c_int32), ("clip_idx", C.c_int32), ("eta", C.c_float)]


class RunSpecC(C.Structure):
    """dsh_run_spec: everything one loop needs beside its options.  Build it with :func:`run_spec`, which fills in ``struct_size``."""
    _fields_ = [("struct_size", C.c_uint32), ("init", C.c_int32), ("masked", C.c_int32), ("start_level", C.c_int32),
                ("invert_from", C.c_int32), ("invert_to", C.c_int32), ("x", C.c_void_p), ("gt", C.c_void_p), ("mask", C.c_void_p),
                ("noise_stack", C.c_void_p), ("n_draws", C.c_int64), ("trace", C.c_void_p),
                ("timesteps", C.POINTER(C.c_int32)), ("n_timesteps", C.c_int32), ("tail_blend", C.c_int32),
                ("row_keys", C.POINTER(C.c_uint64)), ("row_seeds", C.POINTER(C.c_uint64)), ("n_rows", C.c_int32), ("solver", C.c_int32),
                ("guidance", C.c_int32), ("guide_space", C.c_int32), ("n_guide_scale", C.c_int32),
                ("guide_batch", C.c_int32), ("guide_frames", C.c_int32), ("guide_channels", C.c_int32),
                ("guide_target", C.c_void_p), ("guide_weight", C.c_void_p), ("guide_vel", C.c_void_p), ("guide_acc", C.c_void_p),
                ("guide_scale", C.POINTER(C.c_float)),
                ("sync_left", C.POINTER(C.c_int32)), ("n_sync", C.c_int32), ("sync_len", C.c_int32)]


class GuideC(C.Structure):
    """dsh_guide: the guidance terms of one op-level launch."""
    _fields_ = [("target", C.c_void_p), ("weight", C.c_void_p), ("vel", C.c_void_p), ("acc", C.c_void_p),
                ("lens_dev", C.c_void_p), ("lens_host", C.POINTER(C.c_int32)), ("scale", C.c_float), ("space", C.c_int32)]


GUIDE_SPACES = {"x_t": 0, "x0": 1}      # the header's two guide-space values


def run_spec(timesteps=(), row_keys=(), row_seeds=(), guide_scale=(), sync_left=(), **fields) -> RunSpecC:
    """A zeroed dsh_run_spec of this binding's size with ``fields`` set; the host arrays are copied and kept alive by the result."""
    s = RunSpecC(struct_size=C.sizeof(RunSpecC), **fields)
    kept, keys = [int(v) for v in timesteps], [int(v) & 0xFFFFFFFFFFFFFFFF for v in row_keys]
    seeds = [int(v) & 0xFFFFFFFFFFFFFFFF for v in row_seeds]
    if seeds and len(seeds) != len(keys):               # (the library reads n_rows entries of both)
        raise ValueError(f"row_seeds needs row_keys and one seed per key ({len(keys)}), got {len(seeds)}")
    scales = [float(v) for v in guide_scale]
    left = [int(v) for v in sync_left]
    s._arrays = ((C.c_int32 * len(kept))(*kept), (C.c_uint64 * len(keys))(*keys), (C.c_uint64 * len(seeds))(*seeds),
                 (C.c_float * len(scales))(*scales), (C.c_int32 * len(left))(*left))
    if left:
        s.sync_left, s.n_sync = s._arrays[4], len(left)
    if scales:
        s.guide_scale, s.n_guide_scale = s._arrays[3], len(scales)
    if kept:
        s.timesteps, s.n_timesteps = s._arrays[0], len(kept)
    if keys:
        s.row_keys, s.n_rows = s._arrays[1], len(keys)
    if seeds:
        s.row_seeds = s._arrays[2]
    return s


# every symbol include/diffsheg_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "dsh_last_error": (C.c_char_p, []),
    "dsh_version": (C.c_char_p, []),
    "dsh_switch_count": (C.c_int32, []),
    "dsh_switch_info": (C.c_int, [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_char_p)]),
    "dsh_switch_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "dsh_create": (C.c_int, [C.POINTER(ModelConfigC), _P, C.POINTER(_P)]),
    "dsh_destroy": (C.c_int, [_P]),
    "dsh_load_tensor": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int32]),
    "dsh_finalize_weights": (C.c_int, [_P]),
    "dsh_weight_bytes": (C.c_int64, [_P]),
    "dsh_set_condition": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P]),
    "dsh_set_condition_ragged": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _P, _P, _P]),
    "dsh_set_modality": (C.c_int, [_P, C.c_int32, _P]),
    "dsh_eval": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "dsh_eval_flops": (C.c_double, [_P]),
    "dsh_profile_enable": (C.c_int, [_P, C.c_int32]),
    "dsh_profile_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dsh_profile_class_info": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]),
    "dsh_debug_copy": (C.c_int, [_P, C.c_char_p, _P]),
    "dsh_sample_run": (C.c_int, [_P, C.POINTER(SamplerOptsC), C.POINTER(RunSpecC)]),
    "dsh_sample_count": (C.c_int, [C.POINTER(SamplerOptsC), C.POINTER(RunSpecC), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dsh_sample_num_draws": (C.c_int64, [C.POINTER(SamplerOptsC), C.c_int32, C.c_int32]),
    "dsh_sample_num_steps": (C.c_int64, [C.POINTER(SamplerOptsC), C.c_int32]),
    "dsh_sample": (C.c_int, [_P, C.POINTER(SamplerOptsC), _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "dsh_sample_set_row_keys": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int32]),
    "dsh_sample_set_row_seeds": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int32]),
    "dsh_sample_set_tail_blend": (C.c_int, [_P, C.c_int32]),
    "dsh_sample_set_start_level": (C.c_int, [_P, C.c_int32]),
    "dsh_sample_num_draws_from": (C.c_int64, [C.POINTER(SamplerOptsC), C.c_int32, C.c_int32, C.c_int32]),
    "dsh_sample_num_steps_from": (C.c_int64, [C.POINTER(SamplerOptsC), C.c_int32, C.c_int32, C.c_int32]),
    "dsh_invert": (C.c_int, [_P, C.POINTER(SamplerOptsC), _P, C.c_int32, _P]),
    "dsh_invert_from": (C.c_int, [_P, C.POINTER(SamplerOptsC), _P, C.c_int32, C.c_int32, _P]),
    "dsh_sample_set_timesteps": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int32]),
    "dsh_sample_set_solver": (C.c_int, [_P, C.c_int32]),
    "dsh_sample_num_draws_subset": (C.c_int64, [C.POINTER(SamplerOptsC), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "dsh_sample_num_steps_subset": (C.c_int64, [C.POINTER(SamplerOptsC), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "dsh_diffusion_table_subset": (C.c_int32, [C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_char_p, C.POINTER(C.c_double), C.c_int32]),
    "dsh_solver_coeffs": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "dsh_masked_start_level": (C.c_int32, [C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "dsh_op_dpm2m_step": (C.c_int, [_P] * 7 + [C.c_int32] * 3 + [C.c_float] * 7 + [C.c_int32] * 7),
    "dsh_set_guidance_scale": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int32]),
    "dsh_set_guidance_schedule": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.c_float, C.c_float]),
    "dsh_diffusion_table": (C.c_int32, [C.c_int32, C.c_int32, C.c_char_p, C.POINTER(C.c_double), C.c_int32]),
    "dsh_timestep_map": (C.c_int32, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "dsh_jump_schedule": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "dsh_interp_time": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32]),
    "dsh_interp_time_ragged": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P]),
    "dsh_inv_standardize": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P]),
    "dsh_axis_angle_to_euler": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int32]),
    "dsh_euler_to_axis_angle": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, C.c_int64, _P, C.c_int32]),
    "dsh_fk_positions": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int32]),
    "dsh_fk_positions_vjp": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int32]),
    "dsh_op_gemm": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "dsh_op_gemm_ex": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P] + [C.c_int32] * 11),
    "dsh_op_gemm_f32_pro": (C.c_int, [_P, C.c_int32] + [_P, C.c_int32, C.c_int32] * 4 + [C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    "dsh_op_gemm_f32_pro_ex": (C.c_int, [_P, C.c_int32] + [_P, C.c_int32, C.c_int32] * 4 + [C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32]),
    "dsh_op_split_pack_weight": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "dsh_debug_last_tl_variant": (C.c_int32, []),
    "dsh_debug_launch_counts": (C.c_int32, [C.POINTER(C.c_int64), C.c_int32, C.c_int32]),
    "dsh_debug_loop_regime": (C.c_int, [_P, _P]),
    "dsh_op_tl_linear": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "dsh_op_tl2_ffn": (C.c_int, [_P] * 12 + [C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32]),
    "dsh_op_tl_aud_tail": (C.c_int, [_P] * 16 + [C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32]),
    "dsh_op_tl_aproj": (C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32]),
    "dsh_op_tl_joint": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    "dsh_op_cross_attention": (C.c_int, [_P, C.POINTER(CrossAttnWeightsC), _P, _P, _P] + [C.c_int32] * 7 + [_P]),
    "dsh_op_linear_attention": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "dsh_op_linear_attention_bf16": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "dsh_op_linear_attention_ragged": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P]),
    "dsh_op_linear_attention_tiled": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32]),
    "dsh_op_layernorm": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "dsh_op_ddim_step": (C.c_int, [_P] * 6 + [C.c_int32] * 3 + [C.c_float] * 4 + [C.c_int32] * 6),
    "dsh_op_philox_randn": (C.c_int, [_P, _P, C.c_int64, C.c_uint64, C.c_uint64]),
    "dsh_op_q_sample": (C.c_int, [_P] * 6 + [C.c_int32] * 6 + [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), _P, C.POINTER(C.c_int32), C.c_uint64]),
    "dsh_op_region_mask": (C.c_int, [_P, C.POINTER(C.c_int32), _P, C.c_int32, C.POINTER(C.c_int32), _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "dsh_op_philox_randn_rows": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "dsh_op_philox_randn_rows_ragged": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                                  C.c_uint64, C.c_int32]),
    "dsh_op_philox_randn_rows_seeded": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), _P]),
    "dsh_op_philox_randn_rows_ragged_seeded": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64),
                                                         C.POINTER(C.c_int32), C.c_uint64, C.c_int32, _P]),
    "dsh_op_chain_handoff": (C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32), _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "dsh_op_window_sync": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _P, C.POINTER(C.c_int32), _P, C.c_int32,
                                     C.c_int32, C.c_int32]),
    "dsh_op_chain_save_tail": (C.c_int, [_P, _P, C.POINTER(C.c_int32), _P, C.POINTER(C.c_int32), _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32]),
    "dsh_op_ddim_step_full": (C.c_int, [_P] * 10 + [C.c_int32] * 3 + [C.c_float] * 6 + [C.c_int32] * 6),
    "dsh_op_ddpm_step": (C.c_int, [_P] * 5 + [C.c_int64] + [C.c_float] * 5 + [C.c_int32] * 4),
    "dsh_op_guidance_grad": (C.c_int, [_P, _P, _P] + [C.c_int32] * 5 + [C.POINTER(GuideC)]),
    "dsh_op_guided_ddim_step": (C.c_int, [_P] * 8 + [C.POINTER(GuideC)] + [C.c_int32] * 3 + [C.c_float] * 10 + [C.c_int32] * 7),
    "dsh_op_guided_ddpm_step": (C.c_int, [_P] * 5 + [C.POINTER(GuideC)] + [C.c_int32] * 3 + [C.c_float] * 6 + [C.c_int32] * 3),
    "dsh_op_undo_step": (C.c_int, [_P, _P, _P, C.c_float, C.c_float, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "dsh_op_level_copy": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, _P, C.c_int64, _P, C.c_int32]),
    "dsh_op_fill_step": (C.c_int, [_P] * 5 + [C.c_int64, C.c_float, C.c_float, C.c_int64, C.c_int32]),
    "dsh_op_store_values_f32": (C.c_int, [_P, _P, C.POINTER(C.c_float), C.c_int32]),
    "dsh_op_zero_padded_frames": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "dsh_op_fill_cols": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int32]),
    "dsh_op_temb": (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int32]),
    "dsh_op_cfg_mix": (C.c_int, [_P, _P] + [C.c_int32] * 6 + [_P, C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, C.c_int32]),
    "dsh_op_cfg_mix_sched": (C.c_int, [_P, _P] + [C.c_int32] * 6 + [_P, C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, C.c_int32,
                                       _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_float, _P]),
    "dsh_op_im2col3": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    "dsh_op_film_fold": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "dsh_op_film_expand": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32]),
    "dsh_op_gather_rows": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "dsh_op_seed_stream": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "dsh_op_pack_expr_track": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P]),
    "dsh_op_layernorm_pre": (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, C.c_int32]),
    "dsh_op_ln_film_silu": (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32]),
    "dsh_op_concat_ln": (C.c_int, [_P, C.c_int32] + [_P, C.c_int32, C.c_int32] * 4 + [C.c_int32, _P, _P, _P, C.c_int32, C.c_int32]),
    "dsh_fgd_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(_P)]),
    "dsh_fgd_destroy": (C.c_int, [_P]),
    "dsh_fgd_load_tensor": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int32]),
    "dsh_fgd_finalize": (C.c_int, [_P]),
    "dsh_fgd_debug_num_layers": (C.c_int32, [_P]),
    "dsh_fgd_debug_packed_layer": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32), _P, _P]),
    "dsh_fgd_encode": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "dsh_op_conv_gemm_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P, _P, C.c_int64] + [C.c_int32] * 6),
    "dsh_batch_metrics_result_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "dsh_op_batch_metrics": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "dsh_denoise_losses_result_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "dsh_op_denoise_losses": (C.c_int, [_P] * 8 + [C.c_int32] * 4 + [C.c_float, _P, _P, _P]),
    "dsh_mel_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(_P)]),
    "dsh_mel_destroy": (C.c_int, [_P]),
    "dsh_mel_num_frames": (C.c_int64, [_P, C.c_int64]),
    "dsh_mel_debug_tables": (C.c_int, [_P, C.POINTER(C.c_int32), _P, _P]),
    "dsh_mel_compute": (C.c_int, [_P, _P, C.c_int32, C.c_int64, _P]),
    "dsh_mel_compute_ragged": (C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P]),
    "dsh_resample_poly_len": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "dsh_op_resample_poly": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    "dsh_op_resample_poly_ragged": (C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    "dsh_op_softmax_attention": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "dsh_op_softmax_attention_ragged": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "dsh_hubert_create": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "dsh_hubert_destroy": (C.c_int, [_P]),
    "dsh_hubert_load_tensor": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int32]),
    "dsh_hubert_finalize": (C.c_int, [_P]),
    "dsh_hubert_debug_packed": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _P, _P, _P]),
    "dsh_hubert_num_frames": (C.c_int64, [_P, C.c_int64]),
    "dsh_hubert_set_chunk_pass": (C.c_int, [_P, C.c_int32]),
    "dsh_hubert_encode": (C.c_int, [_P, _P, C.c_int32, C.c_int64, _P]),
    "dsh_hubert_encode_ragged": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.POINTER(C.c_int64), _P]),
    "dsh_hubert_set_precision": (C.c_int, [_P, C.c_int32]),
    "dsh_hubert_debug_tap": (C.c_int, [_P, _P]),
    "dsh_op_gemm_bf16_pro": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "dsh_op_softmax_attention_bf16": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "dsh_op_softmax_attention_bf16_ragged": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "dsh_op_pos_conv": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "dsh_op_pos_conv_ragged": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "dsh_op_conv0_ln_gelu": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "dsh_op_conv_ln_gelu": (C.c_int, [_P, _P] + [C.c_int32] * 6 + [_P, _P, _P, _P, _P]),
}

METRICS_HEADER = 5      # DSH_METRICS_HEADER: 8-byte words in front of the per-group diversity values of dsh_op_batch_metrics
LOSS_HEADER, LOSS_COLS = 8, 7      # the header's loss macros: batch scalars in front of, and terms per row of, dsh_op_denoise_losses

# index -> name of the entries of dsh_debug_launch_counts (include/diffsheg_hip.h); eval_streams .. sample_pipe and gemm_tile_pick are
# values, not counts
# (indices 4 and 7 are retired: their kernel forms were removed, the counts stay 0; the names keep the indices fixed)
LAUNCH_FAMILIES = ("tl1", "tl2_loop", "tl2_roll", "tl2_roll_hl", "tl4", "tls", "ffn_fused", "ffn_fused_sty", "attn_mfma", "attn_rowmajor",
                   "gemm_f32_fewrow", "gemm_f32_tiled", "gemm_f32_pro", "eval_streams", "sample_streams", "sample_graph", "sample_pipe",
                   "gemv", "gemm_bf16_tiled", "gemm_tile_pick", "gemm_f32_split", "gemm_f32_split_128")


def launch_counts(reset: bool = False) -> dict:
    """Test helper: launches per kernel family since the last reset (host-side counters of the library), by name."""
    arr = (C.c_int64 * len(LAUNCH_FAMILIES))()
    n = lib().dsh_debug_launch_counts(arr, len(LAUNCH_FAMILIES), int(reset))
    if n != len(LAUNCH_FAMILIES):
        raise DshError(f"dsh_debug_launch_counts reports {n} entries, this binding knows {len(LAUNCH_FAMILIES)}")
    return dict(zip(LAUNCH_FAMILIES, arr))


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DshError(f"{LIB_PATH} not found: the HIP extension is not built and there is no CPU fallback "
                           f"(run `make -C diffsheg_amd/csrc` or __graft_entry__.build())")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)          # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int, what: str = "") -> int:
    if rc < 0:
        msg = lib().dsh_last_error()
        raise DshError(f"{what or 'libdiffsheg_hip'} failed ({rc}): {msg.decode() if msg else '?'}")
    return rc
