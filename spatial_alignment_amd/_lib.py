"""ctypes binding of libgpsa_hip.so (the C ABI declared in include/gpsa_hip.h).

The product path has no CPU fallback: if the shared library is missing, or no HIP device is
visible when an op is called, this raises.  (tests/ may inject a fake ``ops`` object to exercise the
host logic on CPU; nothing in this package does.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgpsa_hip.so")

_vp, _i, _ll, _d = C.c_void_p, C.c_int, C.c_longlong, C.c_double

# name -> (restype, argtypes); mirrors include/gpsa_hip.h exactly
SIGNATURES = {
    "gpsa_version": (_i, []),
    "gpsa_build_arch": (C.c_char_p, []),
    "gpsa_source_hash": (C.c_char_p, []),
    "gpsa_kmat": (_i, [_i, _i, _i, _vp, _i, _vp, _ll, _i, _vp, _vp, _d, _vp, _vp]),
    "gpsa_kmat_bwd_workspace": (_ll, [_i, _i, _ll, _i]),
    "gpsa_kmat_bwd": (_i, [_i, _i, _i, _vp, _i, _vp, _ll, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_gemm_workspace": (_ll, [_i, _i, _i, _i, _i]),
    "gpsa_gemm": (_i, [_i, _i, _i, _i, _i, _ll, _d, _vp, _ll, _ll, _vp, _ll, _ll, _d, _vp, _ll, _ll,
                       _i, _i, _vp, _ll, _vp]),
    "gpsa_omega_fwd": (_i, [_vp, _i, _i, _d, _vp, _vp]),
    "gpsa_omega_bwd": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "gpsa_omega_fwd2": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _d, _vp]),
    "gpsa_omega_bwd2": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "gpsa_chol_f64": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "gpsa_tri_inv_f64": (_i, [_vp, _vp, _i, _i, _vp]),
    "gpsa_chol_inv_f64": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "gpsa_experiment_split_bf16_product": (_i, [_vp, _vp, _i, _ll, _i, _i, _vp, _vp]),
    "gpsa_experiment_split_bf16_rate": (_i, [_i, _i, _vp, _vp]),
    "gpsa_chol_inv_sel_f64": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "gpsa_chol_inv_blocked_workspace": (_ll, [_i, _i]),
    "gpsa_chol_inv_blocked_f64": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_quadform_workspace": (_ll, [_i, _i, _ll, _i]),
    "gpsa_quadform_fwd": (_i, [_i, _i, _vp, _vp, _i, _ll, _i, _vp, _vp, _ll, _vp]),
    "gpsa_quadform_bwd_alpha": (_i, [_i, _i, _vp, _vp, _vp, _i, _ll, _i, _vp, _vp, _ll, _vp]),
    "gpsa_quadform_fwd_keep": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp]),
    "gpsa_quadform_bwd_alpha_kept": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp]),
    "gpsa_quadform_bwd_omega": (_i, [_i, _i, _vp, _vp, _i, _ll, _i, _vp, _vp, _ll, _vp]),
    "gpsa_quadform_bwd_omega_takes_delta": (_i, [_i, _ll]),
    "gpsa_quadform_bwd_omega_delta_f32": (_i, [_i, _vp, _vp, _vp, _i, _ll, _i, _vp, _vp, _d, _vp, _ll, _vp]),
    "gpsa_quadform_bwd_omega_x3_workspace": (_ll, [_i, _ll, _i]),
    "gpsa_quadform_bwd_omega_x3": (_i, [_i, _i, _vp, _vp, _i, _ll, _i, _vp, _vp, _ll, _vp]),
    "gpsa_quadform_bwd_omega_delta_x3": (_i, [_i, _vp, _vp, _vp, _i, _ll, _i, _vp, _vp, _d, _vp, _ll, _vp]),
    "gpsa_whiten_workspace": (_ll, [_i]),
    "gpsa_whiten_f64": (_i, [_vp, _i, _vp, _i, _ll, _i, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_panel_mm": (_i, [_i, _i, _i, _vp, _vp, _i, _ll, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_col_axpy": (_i, [_i, _vp, _vp, _vp, _d, _i, _ll, _vp, _vp]),
    "gpsa_data_sample_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _vp]),
    "gpsa_data_sample_bwd": (_i, [_vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _vp, _i, _vp, _vp, _ll, _vp]),
    "gpsa_warp_sample_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "gpsa_warp_sample_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _ll, _vp]),
    "gpsa_mean_resid_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _d, _vp, _vp, _vp]),
    "gpsa_mean_resid_bwd": (_i, [_vp, _vp, _vp, _i, _i, _d, _vp, _vp, _vp, _vp, _vp]),
    "gpsa_loglik_fwd": (_i, [_vp, _vp, _vp, _i, _ll, _i, _vp, _vp, _ll, _vp]),
    "gpsa_loglik_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_bdot": (_i, [_i, _vp, _ll, _vp, _ll, _ll, _i, _vp, _vp, _ll, _vp]),
    "gpsa_add_diag": (_i, [_i, _vp, _i, _i, _d, _vp]),
    "gpsa_mvn_kl_fwd": (_i, [_vp, _vp, _vp, _ll, _vp, _ll, _vp, _vp, _i, _i, _vp, _vp]),
    "gpsa_mvn_kl_bwd": (_i, [_vp, _vp, _vp, _ll, _vp, _ll, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "gpsa_mvn_kl_grouped_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "gpsa_mvn_kl_grouped_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp,
                                     _vp]),
    "gpsa_elbo_fwd": (_i, [_vp, _i, _vp, _i, _d, _vp, _vp]),
    "gpsa_elbo_bwd": (_i, [_vp, _i, _i, _d, _vp, _vp, _vp]),
    "gpsa_kmeans_workspace": (_ll, [_ll, _i, _i]),
    "gpsa_kmeans_assign": (_i, [_vp, _ll, _i, _vp, _i, _vp, _vp, _vp]),
    "gpsa_kmeans_update": (_i, [_vp, _vp, _ll, _i, _i, _vp, _vp, _vp, _ll, _vp]),
}

MAX_MODS = 4  # GPSA_MAX_MODS


class StepDesc(C.Structure):
    """gpsa_step_desc (include/gpsa_hip.h)"""
    _fields_ = [
        ("n_views", _i), ("n_dims", _i), ("n_mods", _i), ("n_samples", _i),
        ("m_x", _i), ("m_g", _i), ("kind_warp", _i), ("kind_data", _i),
        ("n_latent", _i * MAX_MODS), ("n_out", _i * MAX_MODS), ("has_lmc", _i * MAX_MODS),
        ("n_rows", _ll * MAX_MODS), ("s_test", _i), ("n_test", _ll * MAX_MODS), ("want_kl", _i),
        ("view_fixed", C.POINTER(_i)), ("view_rows", C.POINTER(_ll)), ("keep_budget_bytes", _ll),
        ("exact_inducing_grad", _i), ("kl_own_lo", _i), ("kl_own_hi", _i), ("contraction", _i),
    ]


class StepParams(C.Structure):
    """gpsa_step_params / gpsa_step_param_grads: the same field order, device pointers"""
    _fields_ = [
        ("Xtilde", _vp), ("delta_G", _vp), ("Omega_sqt_G", _vp), ("warp_ls", _vp), ("warp_var", _vp),
        ("slopes", _vp), ("intercepts", _vp), ("Gtilde", _vp), ("data_ls", _vp), ("data_var", _vp),
        ("Omega_sqt_F", _vp * MAX_MODS), ("delta_F", _vp * MAX_MODS), ("W", _vp * MAX_MODS),
    ]


class StepParamGrads(C.Structure):
    _fields_ = [
        ("Xtilde", _vp), ("delta_G", _vp), ("Omega_sqt_G", _vp), ("warp_ls", _vp), ("warp_var", _vp),
        ("Gtilde", _vp), ("data_ls", _vp), ("data_var", _vp),
        ("Omega_sqt_F", _vp * MAX_MODS), ("delta_F", _vp * MAX_MODS), ("W", _vp * MAX_MODS),
    ]


class StepIO(C.Structure):
    _fields_ = [
        ("X", _vp * MAX_MODS), ("eps_G", _vp), ("eps_F", _vp * MAX_MODS), ("G_test", _vp * MAX_MODS),
        ("eps_F_test", _vp * MAX_MODS), ("G_means", _vp * MAX_MODS), ("G_samples", _vp * MAX_MODS),
        ("F_latent", _vp * MAX_MODS), ("F_obs", _vp * MAX_MODS), ("F_latent_test", _vp * MAX_MODS),
        ("F_obs_test", _vp * MAX_MODS), ("mu_z", _vp), ("kl", _vp), ("flag", _vp), ("keep_products", _i),
        ("reuse_mm", _i), ("fuse_elbo", _i), ("Y", _vp * MAX_MODS), ("noise_u", _vp * MAX_MODS),
        ("ll_part", _vp * MAX_MODS), ("F_fused_T", _vp * MAX_MODS), ("bwd_acc", _vp), ("bwd_acc_mode", _i),
        ("f_event", _vp), ("loss_src", _vp), ("loss_dst", _vp), ("skip_missing", _i),
    ]


class StepOutGrads(C.Structure):
    _fields_ = [
        ("dG_means", _vp * MAX_MODS), ("dG_samples", _vp * MAX_MODS), ("dF_latent", _vp * MAX_MODS),
        ("dF_obs", _vp * MAX_MODS), ("dF_latent_test", _vp * MAX_MODS), ("dF_obs_test", _vp * MAX_MODS),
        ("dkl", _vp), ("gloss", _vp),
    ]


_pp = C.POINTER(_vp)  # host array of device pointers

SIGNATURES.update({
    "gpsa_kmat_batched": (_i, [_i, _vp, _ll, _i, _vp, _ll, _ll, _i, _vp, _vp, _i, C.POINTER(_ll), _i, _d, _vp, _ll, _vp]),
    "gpsa_kmat_bwd_batched_workspace": (_ll, [_i, _ll, _i, _i]),
    "gpsa_kmat_bwd_batched": (_i, [_i, _vp, _ll, _i, _vp, _ll, _ll, _i, _vp, _vp, _i, C.POINTER(_ll), _i, _vp, _ll, _i,
                                   _vp, _ll, _vp, _vp, _ll, _vp]),
    "gpsa_kmat_bwd_x64": (_i, [_i, _vp, _i, _vp, _ll, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_kmat_bwd_x64_f64": (_i, [_i, _vp, _i, _vp, _ll, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_kmat_bwd_x64_f64_axpy": (_i, [_i, _vp, _i, _vp, _ll, _i, _vp, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp, _ll,
                                        _vp]),
    "gpsa_exact_dkuu_workspace": (_ll, [_i, _ll]),
    "gpsa_exact_dkuu_f64": (_i, [_vp, _vp, _vp, _i, _ll, _vp, _vp, _ll, _vp]),
    "gpsa_longk_f64_workspace": (_ll, [_i, _ll, _i]),
    "gpsa_longk_f64": (_i, [_i, _vp, _vp, _vp, _i, _i, _ll, _ll, _i, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_kmat_bwd_x64_axpy": (_i, [_i, _vp, _i, _vp, _ll, _i, _vp, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp, _ll,
                                    _vp]),
    "gpsa_thin_update_f32": (_i, [_vp, _i, _i, _vp, _ll, _vp, _vp]),
    "gpsa_whiten_f64_dual": (_i, [_vp, _vp, _i, _ll, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_whiten_gen_f64_dual": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _ll, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_whiten_axpy_f32": (_i, [_vp, _vp, _i, _ll, _vp, _vp, _d, _vp, _vp, _ll, _vp]),
    "gpsa_whiten_batched_f64": (_i, [_vp, _ll, _vp, _i, _ll, _ll, _vp, _vp, _i, _vp, _ll, _vp]),
    "gpsa_quadform_fwd_keep_batched_f64": (_i, [_vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "gpsa_quadform_bwd_alpha_kept_batched_f64": (_i, [_vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _i, _vp]),
    "gpsa_col_axpy_batched_f64": (_i, [_vp, _vp, _vp, _d, _i, _ll, _vp, _i, _vp]),
    "gpsa_gram_batched_workspace": (_ll, [_i, _ll, _i, _i]),
    "gpsa_gram_batched_f64": (_i, [_vp, _vp, _i, _ll, _i, _vp, _i, _vp, _ll, _vp]),
    "gpsa_mvn_kl_grouped_bwd_acc": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i,
                                         _vp]),
    "gpsa_mvn_kl_grouped_fwd_slices": (_i, [_i]),
    "gpsa_mvn_kl_grouped_fwd_sliced": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpsa_step_create": (_vp, [C.POINTER(StepDesc)]),
    "gpsa_step_describe": (_i, [C.POINTER(StepDesc), C.POINTER(_ll)]),
    "gpsa_step_destroy": (None, [_vp]),
    "gpsa_step_saved_bytes": (_ll, [_vp]),
    "gpsa_step_saved_bytes_nokeep": (_ll, [_vp]),
    "gpsa_quadform_keep_f32_workspace": (_ll, [_i, _i]),
    "gpsa_quadform_fwd_keep_f32": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_quadform_keep_f32_bytes": (_ll, [_i, _ll, _i]),
    "gpsa_quadform_bwd_alpha_kept_f32": (_i, [_vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp]),
    "gpsa_lmc_loglik_workspace": (_ll, [_ll, _i, _i, _i]),
    "gpsa_lmc_loglik_fused_f32": (_i, [_vp, _vp, _vp, _vp, _i, _ll, _i, _i, _vp, _i, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_quadform_elbo_parts": (_i, []),
    "gpsa_quadform_elbo_f32_workspace": (_ll, [_i, _ll, _i]),
    "gpsa_quadform_elbo_f32": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _ll, _vp]),
    "gpsa_quadform_elbo_takes_delta": (_i, [_i]),
    "gpsa_quadform_elbo_x3_f32_workspace": (_ll, [_i, _ll, _i]),
    "gpsa_quadform_elbo_x3_f32": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _ll, _vp]),
    "gpsa_quadform_elbo_delta_x3_f32": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _vp,
                                             _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_quadform_elbo_delta_f32": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp, _ll, _vp]),
    "gpsa_step_scratch_bytes": (_ll, [_vp]),
    "gpsa_step_bwd_acc_bytes": (_ll, [_vp]),
    "gpsa_step_n_kl": (_i, [_vp]),
    "gpsa_step_n_factorised": (_i, [_vp]),
    "gpsa_step_eps_g_numel": (_ll, [_vp]),
    "gpsa_step_batch_layout": (_i, [_vp, C.POINTER(_ll)]),
    "gpsa_step_graph": (_i, [_vp, _i, C.POINTER(_ll)]),
    "gpsa_step_early_backwards": (_ll, [_vp]),
    "gpsa_stream_capture_id": (C.c_ulonglong, [_vp]),
    "gpsa_step_timing": (_i, [_vp, _i]),
    "gpsa_step_timing_read": (_i, [_vp, _vp, _i]),
    "gpsa_step_forward": (_i, [_vp, C.POINTER(StepParams), C.POINTER(StepIO), _vp, _vp, _i, _vp]),
    "gpsa_step_backward": (_i, [_vp, C.POINTER(StepParams), C.POINTER(StepIO), C.POINTER(StepOutGrads), _vp, _vp,
                                C.POINTER(StepParamGrads), _vp]),
    "gpsa_elbo_loss_fwd": (_i, [_i, _pp, _pp, _pp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i), _vp, _i, _d, _vp,
                                _vp, _vp, _ll, _vp]),
    "gpsa_elbo_loss_bwd": (_i, [_i, _pp, _pp, _pp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i), _vp, _i, _d, _pp, _pp,
                                _vp, _i, _vp, _vp, _ll, _vp]),
    "gpsa_elbo_loss_fused_fwd": (_i, [_i, _pp, _pp, _pp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i), _pp, _i, _vp, _i,
                                      _d, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_elbo_loss_fused_bwd": (_i, [_i, _pp, _pp, _pp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i), _pp, _i, _vp, _i,
                                      _d, _pp, _pp, _vp, _i, _vp, _vp, _ll, _vp]),
    "gpsa_elbo_fused_post": (_i, [_vp, _vp, _vp, _i, _ll, _i, _vp, _vp, _i, _vp, _vp, _ll, _vp]),
    "gpsa_step_fused": (_i, [_vp, _i]),
    "gpsa_step_contraction": (_i, [_vp, _i]),
    "gpsa_adam_step": (_i, [_i, _pp, _pp, _pp, _pp, C.POINTER(_ll), _d, _d, _d, _d, _vp, _vp]),
    "gpsa_row_sample_gather": (_i, [_i, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_ll), C.c_ulonglong, _vp, _pp,
                                    C.POINTER(_i), _pp, C.POINTER(_i), _pp, _pp, _pp, _vp]),
    "gpsa_elbo_loss_weighted_fwd": (_i, [_i, _pp, _pp, _pp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i),
                                         C.POINTER(_i), _pp, _pp, _vp, _i, _d, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_elbo_loss_weighted_bwd": (_i, [_i, _pp, _pp, _pp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i),
                                         C.POINTER(_i), _pp, _pp, _vp, _i, _d, _pp, _pp, _vp, _i, _vp, _vp, _ll, _vp]),
    "gpsa_quadform_elbo_skip_f32": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _ll, _vp]),
    "gpsa_quadform_elbo_delta_skip_f32": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _vp,
                                               _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_count_observed_workspace": (_ll, []),
    "gpsa_count_observed": (_i, [_i, _pp, C.POINTER(_ll), C.POINTER(_i), C.POINTER(_i), _pp, _pp, _vp, _ll, _vp]),
    "gpsa_elbo_loss_skip_fwd": (_i, [_i, _pp, _pp, _pp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i), _pp, _i,
                                     C.POINTER(_i), _pp, _pp, _pp, _vp, _i, _d, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_elbo_loss_skip_bwd": (_i, [_i, _pp, _pp, _pp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i), _pp, _i,
                                     C.POINTER(_i), _pp, _pp, _pp, _vp, _i, _d, _pp, _pp, _vp, _i, _vp, _vp, _ll, _vp]),
    "gpsa_lmc_loglik_fused_skip_f32": (_i, [_vp, _vp, _vp, _vp, _i, _ll, _i, _i, _vp, _i, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_predict_moments_f32": (_i, [_vp, _vp, _vp, _vp, _ll, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp]),
    "gpsa_predict_counts_f32": (_i, [_vp, _vp, _vp, _vp, _ll, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the warp as a function of the point: mean / Jacobian / determinant and the Newton inverse (csrc/warp_field.hip)
    "gpsa_warp_field_f64": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _vp, _vp, _vp, _vp]),
    "gpsa_warp_invert_f64": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _ll, _i, _i, _vp, _vp, _vp]),
    # neighbour statistics: exact kNN and the neighbours' weighted average (csrc/neighbors.hip)
    "gpsa_knn_workspace": (_ll, [_ll, _ll, _i, _i]),
    "gpsa_knn_f64": (_i, [_vp, _ll, _vp, _ll, _i, _i, _i, _i, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_knn_average_f32": (_i, [_vp, _vp, _ll, _i, _vp, _ll, _i, _i, _vp, _vp]),
    "gpsa_knn_average_f64": (_i, [_vp, _vp, _ll, _i, _vp, _ll, _i, _i, _vp, _vp]),
    # count preprocessing: margins, deviance, residual transforms, per-view z-score (csrc/counts.hip)
    "gpsa_count_workspace": (_ll, [_ll, _ll]),
    "gpsa_count_margins_f32": (_i, [_vp, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_count_deviance_f32": (_i, [_vp, _ll, _ll, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_count_transform_f32": (_i, [_i, _vp, _ll, _ll, _vp, _vp, _d, _d, _d, _d, _vp, _vp]),
    "gpsa_standardize_views_f32": (_i, [_vp, _ll, _ll, C.POINTER(_ll), _i, _vp, _vp, _vp, _ll, _vp]),
    # ... from a CSR matrix on the device (csrc/counts_sparse.hip); crow / rows are DEVICE int64 arrays
    "gpsa_count_csr_workspace": (_ll, [_ll, _ll]),
    "gpsa_csr_check": (_i, [_vp, _vp, _vp, _ll, _ll, _ll, _vp, _vp, _ll, _vp]),
    "gpsa_count_margins_csr_f32": (_i, [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_count_deviance_csr_f32": (_i, [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_csr_gather_dense_f32": (_i, [_vp, _vp, _vp, _ll, _ll, _ll, _vp, _ll, _vp, _ll, _vp, _vp]),
    # per-view column moments, dense and CSR (csrc/moments.hip); view_off is a HOST int64 array
    "gpsa_column_moments_workspace": (_ll, [_ll, _ll, _i]),
    "gpsa_column_moments_csr_workspace": (_ll, [_ll, _ll, _i]),
    "gpsa_column_moments_f32": (_i, [_i, _vp, _ll, _ll, _vp, C.POINTER(_ll), _i, _vp, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_column_moments_csr_f32": (_i, [_i, _vp, _vp, _vp, _vp, _ll, _ll, _ll, _vp, C.POINTER(_ll), _i, _vp, _vp, _vp,
                                         _vp, _vp, _ll, _vp]),
    # exact GP regression: covariance assembly, the LML gradient's fused reduction, the fused predictive mean (csrc/gpr.hip)
    "gpsa_gpr_cov_f64": (_i, [_i, _vp, _ll, _vp, _ll, _i, _vp, _i, _i, _d, _vp, _vp]),
    "gpsa_gpr_lml_grad_workspace": (_ll, [_ll, _i]),
    "gpsa_gpr_lml_grad_f64": (_i, [_i, _vp, _ll, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_gpr_mean_f64": (_i, [_i, _vp, _ll, _vp, _ll, _i, _vp, _i, _vp, _i, _vp, _vp]),
    # optimal-transport slice alignment: distances, expression rows and cost, the outer step's cost, the Sinkhorn sweeps,
    # the plan (csrc/ot.hip); eps is a DEVICE double
    "gpsa_ot_dist_f64": (_i, [_vp, _ll, _i, _vp, _vp]),
    "gpsa_ot_sqmatvec_f64": (_i, [_vp, _ll, _ll, _vp, _vp, _vp]),
    "gpsa_ot_expr_rows_workspace": (_ll, [_ll]),
    "gpsa_ot_expr_rows_f32": (_i, [_i, _vp, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_ot_expr_cost_f64": (_i, [_i, _vp, _ll, _ll, _vp, _vp, _vp]),
    "gpsa_ot_cost_workspace": (_ll, [_ll, _ll]),
    "gpsa_ot_cost_f64": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _d, _ll, _ll, _vp, _vp, _ll, _vp]),
    "gpsa_ot_sinkhorn_workspace": (_ll, [_ll, _ll]),
    "gpsa_ot_sinkhorn_f64": (_i, [_vp, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _i, _vp, _ll, _vp]),
    "gpsa_ot_plan_workspace": (_ll, [_ll, _ll]),
    "gpsa_ot_plan_f64": (_i, [_vp, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp]),
    # histology images: the pixel modality out of an image, an image read at any coordinates (csrc/image.hip); bbox is a
    # HOST array of four doubles
    "gpsa_image_select_workspace": (_ll, [_ll, _ll, _i]),
    "gpsa_image_select_count_u8": (_i, [_vp, _ll, _ll, _i, _i, _i, C.c_float, _i, C.POINTER(_d), _vp, _ll, _vp]),
    "gpsa_image_select_count_f32": (_i, [_vp, _ll, _ll, _i, _i, _i, C.c_float, _i, C.POINTER(_d), _vp, _ll, _vp]),
    "gpsa_image_select_write_u8": (_i, [_vp, _ll, _ll, _i, _i, _i, C.c_float, _i, C.POINTER(_d), _vp, _ll, _vp, _vp, _ll,
                                        _vp]),
    "gpsa_image_select_write_f32": (_i, [_vp, _ll, _ll, _i, _i, _i, C.c_float, _i, C.POINTER(_d), _vp, _ll, _vp, _vp, _ll,
                                         _vp]),
    "gpsa_image_sample_u8": (_i, [_vp, _ll, _ll, _i, _vp, _ll, _i, C.c_float, _vp, _vp, _vp]),
    "gpsa_image_sample_f32": (_i, [_vp, _ll, _ll, _i, _vp, _ll, _i, C.c_float, _vp, _vp, _vp]),
    # spatial autocorrelation: the weight graph in CSR, its sums, the permuted Moran / Geary numerators (csrc/autocorr.hip)
    "gpsa_graph_workspace": (_ll, [_ll]),
    "gpsa_graph_merge_count": (_i, [_vp, _vp, _vp, _ll, _i, _i, _vp, _vp]),
    "gpsa_graph_merge_write": (_i, [_vp, _vp, _vp, _ll, _i, _i, _i, _vp, _ll, _vp, _vp, _vp]),
    "gpsa_graph_check_f64": (_i, [_vp, _vp, _vp, _ll, _ll, _vp, _vp, _ll, _vp]),
    "gpsa_graph_sums_f64": (_i, [_vp, _vp, _vp, _vp, _vp, _ll, _ll, _vp, _vp, _ll, _vp]),
    "gpsa_autocorr_perm_workspace": (_ll, [_ll, _ll, _ll]),
    "gpsa_autocorr_perm_f64": (_i, [_vp, _ll, _ll, _vp, _vp, _vp, _ll, _vp, _ll, _i, _vp, _vp, _vp, _ll, _vp]),
    # rigid pre-registration: the score of K candidate transforms of one slice against another (csrc/register.hip)
    "gpsa_rigid_scores_workspace": (_ll, [_ll, _ll, _ll, _i, _i, _i]),
    "gpsa_rigid_scores_f64": (_i, [_vp, _vp, _ll, _vp, _vp, _ll, _i, _vp, _ll, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _ll,
                                   _vp]),
    # expression PCA: the covariance's Gram and the projection on the components (csrc/pca.hip); view_off is a HOST array
    "gpsa_pca_gram_groups": (_i, [_ll, _ll]),
    "gpsa_pca_gram_workspace": (_ll, [_ll, _ll, _i]),
    "gpsa_pca_gram_f32": (_i, [_vp, _ll, _ll, _vp, _vp, C.POINTER(_ll), _i, _vp, _vp, _ll, _vp]),
    "gpsa_pca_project_f32": (_i, [_vp, _ll, _ll, _vp, _vp, C.POINTER(_ll), _i, _vp, _i, _vp, _i, _vp]),
    # count outputs (model.likelihood): the Poisson term
    "gpsa_lgamma_sum_workspace": (_ll, []),
    "gpsa_lgamma_sum": (_i, [_i, _pp, C.POINTER(_ll), C.POINTER(_i), C.POINTER(_i), _pp, _i, _pp, _vp, _ll, _vp]),
    "gpsa_elbo_loss_pois_fwd": (_i, [_i, _pp, _pp, _pp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i), _pp, _i,
                                     C.POINTER(_i), _pp, _pp, _pp, C.POINTER(_i), _pp, _pp, _i, _vp, _i, _d, _vp, _vp,
                                     _vp, _ll, _vp]),
    "gpsa_elbo_loss_pois_bwd": (_i, [_i, _pp, _pp, _pp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i), _pp, _i,
                                     C.POINTER(_i), _pp, _pp, _pp, C.POINTER(_i), _pp, _pp, _i, _vp, _i, _d, _pp, _pp,
                                     _vp, _i, _vp, _vp, _ll, _vp]),
    "gpsa_quadform_elbo_pois_f32": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _i, _vp, _ll, _vp]),
    "gpsa_quadform_elbo_delta_pois_f32": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _vp,
                                               _vp, _vp, _vp, _vp, _i, _vp, _ll, _vp]),
    "gpsa_lmc_loglik_fused_pois_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _ll, _i, _i, _vp, _i, _vp, _vp, _vp, _ll, _vp]),
    "gpsa_step_likelihood": (_i, [_vp, _i, _i, _vp]),
    # count outputs (model.likelihood): the negative binomial term, a dispersion per output
    "gpsa_nb_const_workspace": (_ll, [_ll, _i, _i]),
    "gpsa_nb_const": (_i, [_i, _pp, C.POINTER(_ll), C.POINTER(_i), _pp, C.POINTER(_i), _pp, _pp, _i, _pp, _pp, _vp, _ll,
                           _vp]),
    "gpsa_quadform_elbo_nb_f32": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _ll, _vp]),
    "gpsa_quadform_elbo_delta_nb_f32": (_i, [_i, _vp, _vp, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _vp,
                                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _ll, _vp]),
    "gpsa_step_dispersion": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "gpsa_lmc_loglik_nb_workspace": (_ll, [_ll, _i, _i, _i]),
    "gpsa_lmc_loglik_fused_nb_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _ll, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _ll,
                                          _vp]),
    "gpsa_elbo_loss_nb_workspace": (_ll, [_i, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i), C.POINTER(_i),
                                          C.POINTER(_i)]),
    "gpsa_elbo_loss_nb_fwd": (_i, [_i, _pp, _pp, _pp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i), _pp, _i,
                                   C.POINTER(_i), _pp, _pp, _pp, C.POINTER(_i), _pp, _pp, _pp, _pp, _i, _vp, _i, _d, _vp,
                                   _vp, _vp, _ll, _vp]),
    "gpsa_elbo_loss_nb_bwd": (_i, [_i, _pp, _pp, _pp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_i), _pp, _i,
                                   C.POINTER(_i), _pp, _pp, _pp, C.POINTER(_i), _pp, _pp, _pp, _pp, _pp, _i, _vp, _i, _d,
                                   _pp, _pp, _vp, _i, _vp, _pp, _vp, _ll, _vp]),
})

LIK_KINDS = {"gaussian": 0, "poisson": 1}  # GPSA_LIK_GAUSSIAN / GPSA_LIK_POISSON: the kinds gpsa_step_likelihood takes
# (a negative binomial modality reaches the step engine through gpsa_step_dispersion)
LIK_NEGBIN = 2  # GPSA_LIK_NEGBIN
# every value of model.likelihood -> its GPSA_LIK_* kind (LIK_KINDS stays the two-entry table it was: what reads it, the
# step engine's setter among them, knows no third kind)
LIK_KIND_OF = dict(LIK_KINDS, negative_binomial=LIK_NEGBIN)

_lib = None


def source_hash():
    """sha256 over the library's sources (csrc/*.hip, *.hpp, include/gpsa_hip.h: names and contents) - what
    __graft_entry__.build() stamps into the library; None when the sources are not next to the package"""
    import glob
    import hashlib

    csrc = os.path.join(_HERE, "csrc")
    header = os.path.join(os.path.dirname(_HERE), "include", "gpsa_hip.h")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")))
    if not files or not os.path.exists(header):
        return None
    h = hashlib.sha256()
    for f in files + [header]:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
        h.update(b"\0")
    return h.hexdigest()


def library_hash(path=None):
    """the stamp inside a built library, read from its bytes (no dlopen), or None"""
    import re

    path = path or LIB_PATH
    if not os.path.exists(path):
        return None
    m = re.search(rb"GPSA_SOURCE_HASH=([0-9a-f]{64}|unstamped)", open(path, "rb").read())
    return m.group(1).decode() if m else None


class GpsaHipError(RuntimeError):
    pass


def load():
    """Load the shared library (once) and attach argtypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GpsaHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == header/library mismatch
        fn.restype = res
        fn.argtypes = args
    want = source_hash()
    got = lib.gpsa_source_hash().decode().split("=", 1)[1]
    if want is not None and got != want and os.environ.get("GPSA_ALLOW_STALE_LIB") != "1":
        raise GpsaHipError(
            f"{LIB_PATH} was built from other sources (stamp {got[:12]}, sources {want[:12]}): rebuild it with "
            "`python -c 'import __graft_entry__ as g; g.build()'`"
        )
    _lib = lib
    return lib


GPSA_EINVAL, GPSA_EWORKSPACE, GPSA_EUNSUPPORTED = -1, -2, -3  # include/gpsa_hip.h


def check(rc, what):
    if rc != 0:
        kind = {-1: "invalid argument", -2: "workspace too small", -3: "unsupported size"}.get(
            rc, f"hipError_t {rc}"
        )
        raise GpsaHipError(f"{what} failed: {kind}")
