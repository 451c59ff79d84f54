"""ctypes binding of libcapgen.so (the C ABI declared in include/capgen.h).

The library is loaded AFTER `import torch`, so its NEEDED libamdhip64.so.7 resolves to
the HIP runtime torch already mapped: device pointers, streams and events are shared
with PyTorch.  There is no fallback: if the library is missing, importing the engine
raises, loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede the dlopen, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CAPGEN_LIB_PATH") or os.path.join(_HERE, "libcapgen.so")  # (diagnostic builds)
ABI_VERSION = 13

F32, BF16 = 0, 1


class capgen_config(C.Structure):
    _fields_ = [
        ("num_vocab", C.c_int32), ("max_length", C.c_int32),
        ("dim_features", C.c_int32), ("dim_positions", C.c_int32),
        ("enc_d", C.c_int32), ("enc_ff", C.c_int32), ("enc_blocks", C.c_int32), ("enc_heads", C.c_int32),
        ("dim_word_embedding", C.c_int32),
        ("dec_d", C.c_int32), ("dec_ff", C.c_int32), ("dec_blocks", C.c_int32), ("dec_heads", C.c_int32),
        ("dropout", C.c_float), ("attention_dropout", C.c_float),
        ("pad_idx", C.c_int32), ("encode_mask", C.c_int32), ("focal_loss", C.c_int32),
        ("split_position", C.c_int32), ("split_image_objects", C.c_int32),
        ("move_first_image_feature", C.c_int32),
        ("dtype", C.c_int32), ("max_batch", C.c_int32), ("max_regions", C.c_int32),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("seed", C.c_uint64),
    ]


class capgen_param_info(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("ndim", C.c_int32), ("rows", C.c_int64), ("cols", C.c_int64),
                ("offset", C.c_int64), ("row_stride", C.c_int64)]


_P = C.c_void_p


class capgen_attn_geom(C.Structure):
    """capgen_attn_geom_t (include/capgen.h): one attention launch's geometry for capgen_debug_attention_geom"""
    _fields_ = [
        ("B", C.c_int32), ("H", C.c_int32), ("Lq", C.c_int32), ("Lk", C.c_int32), ("dk", C.c_int32),
        ("q", _P), ("q_ld", C.c_int64), ("q_bs", C.c_int64),
        ("k", _P), ("k_ld", C.c_int64), ("k_bs", C.c_int64),
        ("v", _P), ("v_ld", C.c_int64), ("v_bs", C.c_int64),
        ("o_ld", C.c_int64), ("o_bs", C.c_int64),
        ("kv_bmod", C.c_int32),
        ("kv_row", _P), ("kv_row_ld", C.c_int64),
        ("key_valid", _P), ("kv_bs", C.c_int64),
        ("key_ids", _P), ("kid_bs", C.c_int64), ("pad_idx", C.c_int32),
        ("causal", C.c_int32), ("q_pos0", C.c_int32),
        ("temperature", C.c_float),
        ("drop_p", C.c_float), ("drop_site", C.c_int32), ("drop_seed", C.c_uint64),
    ]


class capgen_decode_constraints(C.Structure):
    """capgen_decode_constraints (include/capgen.h); banned is a host array the call copies"""
    _fields_ = [("no_repeat_ngram", C.c_int32), ("min_length", C.c_int32), ("end_id", C.c_int32),
                ("repetition_penalty", C.c_float), ("banned", C.POINTER(C.c_int32)), ("n_banned", C.c_int32)]


def decode_constraints(no_repeat_ngram=0, min_length=0, end_id=-1, repetition_penalty=1.0, banned=()):
    """The struct for capgen_set_decode_constraints / capgen_debug_constrain_logits (it keeps its list alive)"""
    ids = [int(w) for w in banned]
    c = capgen_decode_constraints(int(no_repeat_ngram), int(min_length), int(end_id), float(repetition_penalty),
                                  None, len(ids))
    if ids:
        c._banned = (C.c_int32 * len(ids))(*ids)
        c.banned = C.cast(c._banned, C.POINTER(C.c_int32))
    return c


ENS_PROB, ENS_LOGPROB = 0, 1
ENS_MODES = {"prob": ENS_PROB, "logprob": ENS_LOGPROB}


class capgen_ensemble(C.Structure):
    """capgen_ensemble (include/capgen.h): members[0] leads; weights is a host array, NULL = equal"""
    _fields_ = [("members", C.POINTER(_P)), ("n_members", C.c_int32), ("weights", C.POINTER(C.c_float)),
                ("mode", C.c_int32)]


def ensemble(handles, weights=None, mode=ENS_PROB):
    """The struct for capgen_ensemble_beam_nbest / capgen_ensemble_sample (it keeps its arrays alive)"""
    hs = [h.value if isinstance(h, C.c_void_p) else h for h in handles]
    e = capgen_ensemble()
    e._members = (_P * len(hs))(*hs)
    e.members, e.n_members, e.mode = C.cast(e._members, C.POINTER(_P)), len(hs), int(mode)
    if weights is not None:
        e._weights = (C.c_float * len(hs))(*[float(w) for w in weights])
        e.weights = C.cast(e._weights, C.POINTER(C.c_float))
    return e


_SIGS = {
    "capgen_last_error": (C.c_char_p, []),
    "capgen_abi_version": (C.c_int, []),
    "capgen_set_knob": (C.c_int, [C.c_char_p, C.c_int, _P]),
    "capgen_debug_build": (C.c_int, []),
    "capgen_param_table": (C.c_int, [C.POINTER(capgen_config), C.POINTER(capgen_param_info), C.c_int,
                                     C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "capgen_create": (C.c_int, [C.POINTER(capgen_config), C.c_int, C.POINTER(_P)]),
    "capgen_destroy": (C.c_int, [_P]),
    "capgen_get_params": (C.c_int, [_P, _P, C.c_int64]),
    "capgen_set_params": (C.c_int, [_P, _P, C.c_int64]),
    "capgen_get_grads": (C.c_int, [_P, _P, C.c_int64]),
    "capgen_set_grads": (C.c_int, [_P, _P, C.c_int64]),
    "capgen_get_adam_state": (C.c_int, [_P, C.POINTER(C.c_int64), _P, _P, C.c_int64]),
    "capgen_set_adam_state": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int64]),
    "capgen_arenas": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64)]),
    "capgen_set_training": (C.c_int, [_P, C.c_int]),
    "capgen_set_graph": (C.c_int, [_P, C.c_int]),
    "capgen_set_decode_log_softmax": (C.c_int, [_P, C.c_int]),
    "capgen_set_lr": (C.c_int, [_P, C.c_float]),
    "capgen_get_lr": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "capgen_set_grad_clip": (C.c_int, [_P, C.c_float]),
    "capgen_last_grad_norm": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "capgen_set_weight_decay": (C.c_int, [_P, C.c_float]),
    "capgen_set_ema": (C.c_int, [_P, C.c_float]),
    "capgen_ema_info": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "capgen_get_ema": (C.c_int, [_P, _P, C.c_int64]),
    "capgen_set_ema_state": (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    "capgen_ema_swap": (C.c_int, [_P]),
    "capgen_forward": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "capgen_backward": (C.c_int, [_P, _P]),
    "capgen_adam_step": (C.c_int, [_P, _P]),
    "capgen_train_step": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "capgen_compute_loss": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "capgen_copy_logits": (C.c_int, [_P, _P, C.c_int64, _P]),
    "capgen_greedy": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P]),
    "capgen_beam": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "capgen_beam_nbest": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P, _P,
                                    _P, _P, _P]),
    "capgen_beam_diverse": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                      C.c_float, C.c_int, _P, _P, _P, _P, _P]),
    "capgen_ensemble_beam_diverse": (C.c_int, [C.POINTER(capgen_ensemble), _P, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, _P, _P, _P, _P, _P]),
    "capgen_debug_beam_group_step": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                               _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "capgen_beam_forced": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P, _P,
                                     C.c_int, _P, _P, _P, _P, _P, _P]),
    "capgen_ensemble_beam_forced": (C.c_int, [C.POINTER(capgen_ensemble), _P, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_float, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P]),
    "capgen_debug_beam_forced_step": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int,
                                                _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "capgen_sample": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64, _P, _P,
                                _P]),
    "capgen_sample_nucleus": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float,
                                        C.c_uint64, _P, _P, _P]),
    "capgen_set_decode_constraints": (C.c_int, [_P, C.POINTER(capgen_decode_constraints)]),
    "capgen_debug_constrain_logits": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int64, C.c_int,
                                                C.POINTER(capgen_decode_constraints), _P]),
    "capgen_ensemble_beam_nbest": (C.c_int, [C.POINTER(capgen_ensemble), _P, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_float, C.c_int, _P, _P, _P, _P, _P]),
    "capgen_ensemble_sample": (C.c_int, [C.POINTER(capgen_ensemble), _P, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                         C.c_float, C.c_int, C.c_float, C.c_uint64, _P, _P, _P]),
    "capgen_debug_ensemble_combine": (C.c_int, [C.POINTER(_P), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int,
                                                _P, _P, _P]),
    "capgen_set_rng_seed": (C.c_int, [_P, C.c_uint64]),
    "capgen_debug_gemm": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_int64, C.c_int, _P, C.c_int64, C.c_int,
                                    _P, C.c_int64, C.c_int, C.c_int, _P, C.c_float, C.c_int, C.c_int, _P]),
    "capgen_debug_gemm_tiled": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P, C.c_int64, C.c_int, _P, _P,
                                          C.c_int64, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int64, _P]),
    "capgen_debug_gemm_tiled_ln": (C.c_int, [C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P,
                                             _P, _P, C.c_int64, C.c_int, _P]),
    "capgen_debug_gemm_variant": (C.c_int, [C.c_int]),
    "capgen_debug_splitk_protocol": (C.c_int, [C.c_int]),
    "capgen_debug_splitk_diag": (C.c_int, [_P, C.c_int]),
    "capgen_debug_gemm_timing_buf": (C.c_int, [_P]),
    "capgen_debug_copy_buffer": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "capgen_train_step_indexed": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P,
                                            _P]),
    "capgen_train_step_weighted": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P,
                                             C.c_int, _P]),
    "capgen_score_captions": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P,
                                        _P]),
    "capgen_debug_score_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    "capgen_debug_score_finish": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P,
                                            _P, _P]),
    "capgen_rl_sample": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "capgen_rl_finish": (C.c_int, [_P, _P, C.c_float, _P, C.c_int, _P]),
    "capgen_debug_attention": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P,
                                         C.c_int, C.c_float, _P, _P, _P, _P, _P, _P, _P]),
    "capgen_debug_attention_bwd_wo": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P,
                                                _P, _P, _P, C.c_float, C.c_int, C.c_uint64, _P]),
    "capgen_debug_qkv_attention": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int,
                                             C.c_float, C.c_int, C.c_uint64, _P]),
    "capgen_debug_cross_attention": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_float,
                                               C.c_int, C.c_uint64, _P]),
    "capgen_debug_attention_geom": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "capgen_debug_attention_head_mean": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "capgen_debug_layernorm_fwd": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, C.c_float, C.c_int, C.c_uint64, _P, _P,
                                             C.c_int, _P, _P, _P, C.c_int64, C.c_int, _P, _P, _P, _P, _P, _P]),
    "capgen_debug_layernorm_bwd": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int, _P,
                                             C.c_float, C.c_int, C.c_uint64, _P, _P, _P, _P, _P, C.c_int, C.c_int64,
                                             _P]),
    "capgen_debug_column_sum": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int64, C.c_float, _P, _P, C.c_int,
                                          C.c_int64, _P]),
    "capgen_debug_stripe_reduce": (C.c_int, [_P, C.c_int, C.c_int64, C.c_int64, _P, C.c_int, C.c_int, _P]),
    "capgen_debug_embedding_gather": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P, C.c_int, _P]),
    "capgen_debug_embedding_scatter_add": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "capgen_debug_pack_encoder_input": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P,
                                                  _P, C.c_int, C.c_int, _P, _P]),
    "capgen_debug_prepare_captions": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    "capgen_debug_cross_entropy_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P]),
    "capgen_debug_ce_finish": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "capgen_debug_cross_entropy_rows_weighted": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P,
                                                           C.c_int, _P]),
    "capgen_debug_ce_finish_weighted": (C.c_int, [_P, C.c_int64, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P,
                                                  _P, _P]),
    "capgen_debug_loss_finalize": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, _P]),
    "capgen_debug_adam": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P, _P,
                                    C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                    C.POINTER(_P), _P]),
    "capgen_debug_adam_scaled": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P,
                                           _P, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                           C.POINTER(_P), _P, _P]),
    "capgen_debug_adam_ex": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P, _P,
                                       C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                       C.POINTER(_P), _P, C.c_float, _P, C.c_float, _P]),
    "capgen_debug_arena_swap": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P]),
    "capgen_debug_grad_norm": (C.c_int, [_P, C.c_int64, C.c_float, C.c_int, _P, C.c_int, _P, _P]),
    "capgen_debug_to_bf16": (C.c_int, [_P, _P, C.c_int64, _P]),
    "capgen_debug_arena_checksum": (C.c_int, [_P, C.c_int64, C.POINTER(C.c_uint64), _P]),
    "capgen_debug_argmax_softmax": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, C.c_int, _P, C.c_int64, C.c_int,
                                              _P]),
    "capgen_debug_sample_softmax": (C.c_int, [_P, C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint32, _P,
                                              C.c_int64, C.c_int, _P, C.c_int64, _P, C.c_int64, C.c_int, _P]),
    "capgen_debug_sample_nucleus": (C.c_int, [_P, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_uint64,
                                              C.c_uint32, _P, C.c_int64, C.c_int, _P, C.c_int64, _P, C.c_int64,
                                              C.c_int, _P, _P]),
    "capgen_debug_slab_argmax": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int64, C.c_int, _P, C.c_int64, _P]),
    "capgen_debug_beam_step_topk": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P,
                                              _P, _P]),
    "capgen_debug_beam_slab_step": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P,
                                              _P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "capgen_debug_beam_step_ended": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P,
                                               _P, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int,
                                               _P]),
    "capgen_debug_beam_finish": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P, _P, _P, _P,
                                           _P]),
    "capgen_debug_rl_rows": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "capgen_debug_rl_image": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "capgen_debug_rl_numer": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "capgen_debug_rl_loss": (C.c_int, [_P, _P, C.c_float, _P, _P, _P]),
    "capgen_debug_rl_grad": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P,
                                       C.c_int, _P]),
    "capgen_debug_gemm_classifier": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64,
                                               _P, _P, C.c_int64, _P, _P, _P]),
    "capgen_dp_unique_id": (C.c_int, [C.c_char_p]),
    "capgen_dp_init": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int]),
    "capgen_dp_set_global_count": (C.c_int, [_P, C.c_float]),
    "capgen_dp_sync_adam_state": (C.c_int, [_P]),
    "capgen_dp_comm_info": (C.c_int, [_P, _P, _P]),
    "capgen_dp_check": (C.c_int, [_P, _P, _P]),
    "capgen_params_checksum": (C.c_int, [_P, _P]),
    "capgen_dp_buckets": (C.c_int, [_P, _P, _P, C.c_int, _P]),
    "capgen_dp_debug_shard": (C.c_int, [_P, C.c_int, C.c_int]),
    "capgen_tune_load": (C.c_int, [C.c_char_p]),
    "capgen_tune_save": (C.c_int, [C.c_char_p]),
    "capgen_tune_live_count": (C.c_int, []),
    "capgen_debug_hazard": (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    "capgen_debug_side_delay": (C.c_int, [C.c_double]),
    "capgen_debug_collectives": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_int]),
    "capgen_debug_stamps": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_char_p, C.c_int]),
    "capgen_scst_rewards": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int64, C.c_double, C.c_double, _P]),
}
EXPORTED = tuple(_SIGS)

# the front hooks that gained `drop_p, drop_site, drop_seed` in front of `stream`: a call written for the
# former signature (three arguments fewer) still works through this binding and means dropout off
_DROP_HOOKS = ("capgen_debug_qkv_attention", "capgen_debug_cross_attention", "capgen_debug_attention_bwd_wo")


def _with_default_drop(fn, nargs):
    def hook(*args):
        if len(args) == nargs - 3:
            args = args[:-1] + (0.0, 0, 0) + args[-1:]
        return fn(*args)
    hook.__name__, hook.argtypes, hook.restype = fn.__name__, fn.argtypes, fn.restype
    return hook


_lib = None


def load():
    """dlopen libcapgen.so once; raises if it was not built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"capgen: {LIB_PATH} is missing — build it with "
                          "`python -c 'import __graft_entry__ as g; g.build()'` (make -C image-caption_amd/csrc)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.capgen_abi_version() != ABI_VERSION:
        raise ImportError("capgen: libcapgen.so ABI version mismatch")
    for name in _DROP_HOOKS:
        setattr(lib, name, _with_default_drop(getattr(lib, name), len(_SIGS[name][1])))
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError("capgen: " + load().capgen_last_error().decode(errors="replace"))


def to_c_config(cfg) -> capgen_config:
    cfg.check_supported()
    c = capgen_config()
    c.num_vocab, c.max_length = cfg.num_vocab, cfg.max_length
    c.dim_features, c.dim_positions = cfg.encode_dim_features, cfg.encode_dim_positions
    c.enc_d, c.enc_ff = cfg.encode_input_size, cfg.encode_hidden_size
    c.enc_blocks, c.enc_heads = cfg.encode_num_blocks, cfg.encode_num_heads
    c.dim_word_embedding = cfg.dim_word_embedding
    c.dec_d, c.dec_ff = cfg.decode_input_size, cfg.decode_hidden_size
    c.dec_blocks, c.dec_heads = cfg.decode_num_blocks, cfg.decode_num_heads
    c.dropout, c.attention_dropout = cfg.dropout, cfg.attention_dropout
    c.pad_idx, c.encode_mask, c.focal_loss = cfg.pad_idx, int(cfg.encode_mask), int(cfg.focal_loss)
    c.split_position = int(cfg.split_position)
    c.split_image_objects = int(cfg.split_image_objects)
    c.move_first_image_feature = int(cfg.move_first_image_feature)
    c.dtype = F32 if cfg.dtype == "fp32" else BF16
    c.max_batch, c.max_regions = cfg.max_batch, cfg.max_regions
    c.lr, c.beta1, c.beta2, c.eps = cfg.learning_rate, cfg.beta1, cfg.beta2, cfg.eps
    c.seed = cfg.seed & 0xFFFFFFFFFFFFFFFF
    return c


def param_table(cfg):
    """[(name, ndim, rows, cols, offset, row_stride)], arena_elems — host-only, no GPU needed."""
    lib = load()
    c = to_c_config(cfg)
    n = C.c_int(0)
    total = C.c_int64(0)
    check(lib.capgen_param_table(C.byref(c), None, 0, C.byref(n), C.byref(total)))
    arr = (capgen_param_info * n.value)()
    check(lib.capgen_param_table(C.byref(c), arr, n.value, C.byref(n), C.byref(total)))
    out = [(p.name.decode(), p.ndim, p.rows, p.cols, p.offset, p.row_stride) for p in arr]
    return out, total.value


TUNE_TABLE = os.path.join(_HERE, "tune_gfx950.txt")


def tune_save(path: str = TUNE_TABLE) -> int:
    """Write every GEMM autotune choice this process knows (tuned or loaded) to `path`."""
    n = load().capgen_tune_save(path.encode())
    if n < 0:
        check(1)
    return n


def tune_load(path: str) -> int:
    """Merge a persisted autotune table (-1: no such file)."""
    return load().capgen_tune_load(path.encode())


def tune_live_count() -> int:
    """GEMM shapes this process tuned live (0 when the persisted table covered every shape)."""
    return load().capgen_tune_live_count()


def hazard_start() -> None:
    """Start logging every launch / event / host sync of the engines (clears the log)."""
    check(load().capgen_debug_hazard(1, None, 0, None))


def hazard_stop() -> None:
    check(load().capgen_debug_hazard(0, None, 0, None))


def hazard_check(cap: int = 8192):
    """(number of unordered conflicting launch pairs since hazard_start, report text)."""
    buf = C.create_string_buffer(cap)
    n = C.c_int(0)
    check(load().capgen_debug_hazard(2, buf, cap, C.byref(n)))
    return n.value, buf.value.decode(errors="replace")


def side_delay(us: float) -> None:
    """Spin `us` microseconds in front of every launch off the critical stream (0 = off)."""
    check(load().capgen_debug_side_delay(float(us)))


def set_knob(name: str, value: int) -> int:
    """Set a run-time switch (capgen_set_knob; name without the CAPGEN_ prefix); returns the old value."""
    old = C.c_int(0)
    check(load().capgen_set_knob(name.encode(), int(value), C.byref(old)))
    return old.value


def debug_build() -> bool:
    """True in the debug library (libcapgen_debug.so, CAPGEN_LIB_PATH)."""
    return bool(load().capgen_debug_build())
