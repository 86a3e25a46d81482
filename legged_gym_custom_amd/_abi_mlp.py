"""ctypes mirror of include/lgx_mlp.h (the C ABI of liblgx_mlp.so) and its loader: the structs, the
constants and the function signatures, with the three tables _cbind.py describes at the end.
rsl_rl/modules/hip_mlp.py holds everything that computes or launches on top of it.

Field order and array sizes must match the header exactly: tests/test_abi.py compares every
field's offset and size, every constant and every parameter count with the compiled header.
"""
import ctypes as C
import os

from . import _cbind

_LIB_PATH = os.environ.get("LGX_MLP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                          "liblgx_mlp.so")
_lib = None
ABI_VERSION = 11
EPI_BIAS, EPI_ELU, EPI_DELU, EPI_ACCUM = 1, 2, 4, 8
TAIL_MAX_LOSSES = 8
TAIL_S8_MAX = 32
COPY_MAX = 16
SPLITK_MAX = 24
GROUP_MAX = 20
TRANSPOSE_MAX = 24
CHAIN_MAX, CHAIN_MAXL, CHAIN_MAXW = 4, 3, 256
CLIP_ADAM_MAX = 65536  # entries of lgx_clip_adam's one-block segment
HEADS_TAIL_ROWS = 32  # rows of one column-sum partial of lgx_loss_heads_tail


class GemmArgs(C.Structure):
    """Mirror of lgx_gemm_args (include/lgx_mlp.h)."""
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int64), ("a_kcontig", C.c_int32),
                ("B", C.c_void_p), ("ldb", C.c_int64), ("b_kcontig", C.c_int32),
                ("C", C.c_void_p), ("ldc", C.c_int64),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("epilogue", C.c_int32),
                ("bias", C.c_void_p), ("act", C.c_void_p), ("ld_act", C.c_int64),
                ("split_k", C.c_int32), ("workspace", C.c_void_p), ("colsum", C.c_void_p),
                ("colsum_ws", C.c_void_p), ("defer_reduce", C.c_int32)]


class SplitkDesc(C.Structure):
    """Mirror of lgx_splitk_desc."""
    _fields_ = [("ws", C.c_void_p), ("colsum_ws", C.c_void_p), ("C", C.c_void_p), ("ldc", C.c_int64),
                ("colsum", C.c_void_p), ("M", C.c_int32), ("N", C.c_int32), ("split", C.c_int32),
                ("epilogue", C.c_int32)]


class HeadArgs(C.Structure):
    """Mirror of lgx_ppo_head_args (include/lgx_mlp.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("mu", "value", "std", "actions", "old_logp", "adv", "target_values",
                                          "returns", "old_mu", "old_sigma")] + \
               [("B", C.c_int32), ("A", C.c_int32), ("clip", C.c_float), ("clipped_value", C.c_int32),
                ("out", C.c_void_p), ("g", C.c_void_p), ("dmu", C.c_void_p), ("dvalue", C.c_void_p),
                ("dstd", C.c_void_p), ("ws", C.c_void_p), ("counter", C.c_void_p), ("kl_dst", C.c_void_p),
                ("accumulate_dstd", C.c_int32)]


class AuxArgs(C.Structure):
    """Mirror of lgx_aux_loss_args."""
    _fields_ = [("p", C.c_void_p), ("a", C.c_void_p), ("L", C.c_int32), ("e", C.c_void_p), ("t", C.c_void_p),
                ("E", C.c_int32), ("B", C.c_int32), ("out", C.c_void_p), ("g", C.c_void_p), ("dp", C.c_void_p),
                ("de", C.c_void_p), ("ws", C.c_void_p), ("counter", C.c_void_p), ("ld_p", C.c_int64)]


class HeadsS8Args(C.Structure):
    """Mirror of lgx_heads_s8_args (pitches in S8 elements)."""
    _fields_ = [("dmu_s8", C.c_void_p), ("ld_dmu", C.c_int64), ("dmu_cs", C.c_void_p),
                ("dvalue_s8", C.c_void_p), ("ld_dvalue", C.c_int64), ("dvalue_cs", C.c_void_p),
                ("de_s8", C.c_void_p), ("ld_de", C.c_int64), ("de_cs", C.c_void_p),
                ("decisions_in", C.c_void_p), ("decisions_out", C.c_void_p)]


class HeadsTailArgs(C.Structure):
    """Mirror of lgx_heads_tail_args (ABI 9: the actor's / critic's last layers fused around the
    PPO head; pitches in S8 elements)."""
    _fields_ = [("y", C.c_void_p), ("ld_y", C.c_int64), ("W", C.c_void_p), ("b", C.c_void_p),
                ("dy", C.c_void_p), ("ld_dy", C.c_int64), ("dy_cs", C.c_void_p),
                ("yc", C.c_void_p), ("ld_yc", C.c_int64), ("Wc", C.c_void_p), ("bc", C.c_void_p),
                ("dyc", C.c_void_p), ("ld_dyc", C.c_int64), ("dyc_cs", C.c_void_p),
                ("mu_out", C.c_void_p), ("value_out", C.c_void_p), ("H", C.c_int32), ("Hc", C.c_int32)]


class TailArgs(C.Structure):
    """Mirror of lgx_ppo_tail_args."""
    _fields_ = [(n, C.c_void_p) for n in ("grads", "params", "exp_avg", "exp_avg_sq")] + \
               [(n, C.c_int64) for n in ("main_lo", "main_hi", "est_lo", "est_hi", "adapt_lo", "adapt_hi",
                                         "kl_index")] + \
               [(n, C.c_float) for n in ("max_norm", "b1_main", "b2_main", "eps_main", "b1_est", "b2_est", "eps_est",
                                         "est_lr")] + \
               [("desired_kl", C.c_double), ("lr64", C.c_void_p), ("lr32", C.c_void_p), ("step_main", C.c_void_p),
                ("step_est", C.c_void_p), ("loss_ptrs", C.c_void_p * TAIL_MAX_LOSSES), ("sums", C.c_void_p),
                ("nloss", C.c_int32), ("ws", C.c_void_p), ("counter", C.c_void_p), ("s8", C.c_void_p),
                ("n_s8", C.c_int32)]


class TailS8Seg(C.Structure):
    """Mirror of lgx_tail_s8_seg."""
    _fields_ = [("p0", C.c_int64), ("N", C.c_int32), ("K", C.c_int32), ("c0", C.c_int32), ("w", C.c_int32),
                ("dst", C.c_void_p), ("ld", C.c_int32), ("packed", C.c_int32)]


class CopyDesc(C.Structure):
    """Mirror of lgx_copy_desc."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("nbytes", C.c_int64), ("dst_stride", C.c_int64)]


class ActHeadArgs(C.Structure):
    """Mirror of lgx_act_head_args."""
    _fields_ = [(n, C.c_void_p) for n in ("mean", "std", "eps", "actions", "mu", "sigma", "logp")] + \
               [("B", C.c_int32), ("A", C.c_int32), ("actions_copy", C.c_void_p), ("step_dev", C.c_void_p),
                ("seed", C.c_uint64), ("env_offset", C.c_int64)]


class TransitionArgs(C.Structure):
    """Mirror of lgx_transition_args."""
    _fields_ = [(n, C.c_void_p) for n in ("rewards", "dones", "time_outs", "values", "rewards_out", "dones_out",
                                          "values_out")] + [("gamma", C.c_float), ("B", C.c_int32)]


class TrackArgs(C.Structure):
    """Mirror of lgx_track_args."""
    _fields_ = [(n, C.c_void_p) for n in ("rewards", "dones", "cur_rew", "cur_len", "rew_ring", "len_ring", "ptr",
                                          "n", "ep_a", "ep_b", "ep_sum", "ep_cnt")] + \
        [("N", C.c_int32), ("na", C.c_int32), ("nb", C.c_int32)]


class TransposeDesc(C.Structure):
    """Mirror of lgx_transpose_desc."""
    _fields_ = [("src", C.c_void_p), ("ld", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32),
                ("dst", C.c_void_p)]


class ChainLayer(C.Structure):
    """Mirror of lgx_chain_layer."""
    _fields_ = [("B", C.c_void_p), ("ldb", C.c_int64), ("C", C.c_void_p), ("ldc", C.c_int64),
                ("K", C.c_int32), ("N", C.c_int32), ("epilogue", C.c_int32), ("bias", C.c_void_p),
                ("act", C.c_void_p), ("ld_act", C.c_int64)]


class ChainDesc(C.Structure):
    """Mirror of lgx_chain_desc."""
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int64), ("rows", C.c_int32), ("nlayers", C.c_int32),
                ("layers", ChainLayer * CHAIN_MAXL)]


class AdaptArgs(C.Structure):
    """Mirror of lgx_adapt_args."""
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int64), ("B", C.c_int32), ("H", C.c_int32), ("P", C.c_int32),
                ("w0", C.c_void_p), ("b0", C.c_void_p), ("C1", C.c_int32),
                ("w1", C.c_void_p), ("b1", C.c_void_p), ("C2", C.c_int32), ("k1", C.c_int32), ("s1", C.c_int32),
                ("w2", C.c_void_p), ("b2", C.c_void_p), ("C3", C.c_int32), ("k2", C.c_int32), ("s2", C.c_int32),
                ("wf", C.c_void_p), ("bf", C.c_void_p), ("NO", C.c_int32),
                ("out", C.c_void_p), ("ldo", C.c_int64)]


class AdaptTrainArgs(C.Structure):
    """Mirror of lgx_adapt_train_args (ABI 9)."""
    _fields_ = [("f", AdaptArgs), ("target", C.c_void_p), ("ldt", C.c_int64), ("gws", C.c_void_p),
                ("loss_ws", C.c_void_p), ("blocks", C.c_int32)]


class GaeArgs(C.Structure):
    """Mirror of lgx_gae_args."""
    _fields_ = [(n, C.c_void_p) for n in ("rewards", "dones", "values", "last_values", "returns", "advantages")] + \
               [("T", C.c_int32), ("N", C.c_int32), ("gamma", C.c_float), ("lam", C.c_float)] + \
               [(n, C.c_void_p) for n in ("moments", "ws", "counter")]


STRUCTS = {
    "lgx_gemm_args": GemmArgs, "lgx_chain_layer": ChainLayer, "lgx_chain_desc": ChainDesc,
    "lgx_adapt_args": AdaptArgs, "lgx_adapt_train_args": AdaptTrainArgs, "lgx_splitk_desc": SplitkDesc,
    "lgx_transpose_desc": TransposeDesc, "lgx_ppo_head_args": HeadArgs, "lgx_aux_loss_args": AuxArgs,
    "lgx_heads_s8_args": HeadsS8Args, "lgx_heads_tail_args": HeadsTailArgs, "lgx_tail_s8_seg": TailS8Seg,
    "lgx_ppo_tail_args": TailArgs, "lgx_copy_desc": CopyDesc, "lgx_act_head_args": ActHeadArgs,
    "lgx_transition_args": TransitionArgs, "lgx_track_args": TrackArgs, "lgx_gae_args": GaeArgs,
}
SIZEOF = {"lgx_mlp_sizeof_gemm_args": "lgx_gemm_args"}  # sizeof export -> typedef

# LGX_ACT_NOISE_STREAM is mirrored by oracle/philox.py (STREAM_ACT): the package never passes it
CONSTANTS = {
    "LGX_MLP_ABI_VERSION": ABI_VERSION,
    "LGX_EPI_BIAS": EPI_BIAS, "LGX_EPI_ELU": EPI_ELU, "LGX_EPI_DELU": EPI_DELU, "LGX_EPI_ACCUM": EPI_ACCUM,
    "LGX_GEMM_GROUP_MAX": GROUP_MAX, "LGX_CHAIN_MAX": CHAIN_MAX, "LGX_CHAIN_MAXL": CHAIN_MAXL,
    "LGX_CHAIN_MAXW": CHAIN_MAXW, "LGX_SPLITK_MAX": SPLITK_MAX, "LGX_TRANSPOSE_MAX": TRANSPOSE_MAX,
    "LGX_CLIP_ADAM_MAX": CLIP_ADAM_MAX, "LGX_HEADS_TAIL_ROWS": HEADS_TAIL_ROWS,
    "LGX_TAIL_MAX_LOSSES": TAIL_MAX_LOSSES, "LGX_TAIL_S8_MAX": TAIL_S8_MAX, "LGX_COPY_MAX": COPY_MAX,
}

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
SIGNATURES = {
    "lgx_mlp_abi_version": (i32, ()),
    "lgx_mlp_sizeof_gemm_args": (i32, ()),
    "lgx_mlp_pick_split": (i32, (i32, i32, i32)),
    "lgx_gemm": (i32, (vp, vp)),
    "lgx_gemm_group": (i32, (vp, i32, vp)),
    "lgx_chain": (i32, (vp, i32, vp)),
    "lgx_adaptation_forward": (i32, (vp, vp)),
    "lgx_adaptation_train": (i32, (vp, vp)),
    "lgx_mlp_pick_split_group": (i32, (vp, vp, vp, i32, vp)),
    "lgx_splitk_reduce_batch": (i32, (vp, i32, vp)),
    "lgx_transpose_batch": (i32, (vp, i32, vp)),
    "lgx_mlp_last_error": (C.c_char_p, ()),
    "lgx_adam_step": (i32, (vp, vp, vp, vp, i64, vp, f32, f32, f32, f32, vp, vp, vp)),
    "lgx_clip_adam": (i32, (vp, vp, vp, vp, i64, vp, f32, f32, f32, f32, vp, f32, vp, vp)),
    "lgx_ppo_head_forward": (i32, (vp, vp)),
    "lgx_ppo_head_backward": (i32, (vp, vp)),
    "lgx_aux_loss_forward": (i32, (vp, vp)),
    "lgx_aux_loss_backward": (i32, (vp, vp)),
    "lgx_loss_heads_forward": (i32, (vp, vp, vp)),
    "lgx_loss_heads_backward": (i32, (vp, vp, vp)),
    "lgx_loss_heads_fused": (i32, (vp, vp, vp, vp)),
    "lgx_loss_heads_tail": (i32, (vp, vp, vp, vp, vp)),
    "lgx_ppo_tail": (i32, (vp, vp)),
    "lgx_copy_batch": (i32, (vp, i32, vp)),
    "lgx_gather_rows": (i32, (vp, i32, vp, i64, vp)),
    "lgx_act_head": (i32, (vp, vp)),
    "lgx_store_transition": (i32, (vp, vp)),
    "lgx_track_episodes": (i32, (vp, vp)),
    "lgx_post_step": (i32, (vp, vp, vp)),
    "lgx_gae": (i32, (vp, vp)),
    "lgx_normalize_advantages": (i32, (vp, i64, vp, C.c_double, vp)),
}
EXPORTED = list(SIGNATURES)


class MlpLibError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        _lib = _cbind.load(_LIB_PATH, "liblgx_mlp", SIGNATURES, STRUCTS, ("lgx_mlp_abi_version", ABI_VERSION), SIZEOF,
                           MlpLibError)
    return _lib


def check(rc, what):
    if rc != 0:
        raise MlpLibError(f"{what}: " + lib().lgx_mlp_last_error().decode())
