"""ctypes binding of ``libssak_hip.so`` (C ABI: ``include/ssak_hip.h``).

torch is used here only as plumbing: device buffers (``tensor.data_ptr()``) and the current HIP stream.
Every wrapper raises ``RuntimeError`` when the library reports a launch failure and ``ValueError`` when
it rejects the arguments -- the exception types the reference's Python call sites would see.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

_DEFAULT_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libssak_hip.so")
_LIB_PATH = os.environ.get("SSAK_HIP_LIB") or _DEFAULT_LIB  # (the override names another build OF THE SAME ABI: A/B runs, instrumented builds)
ABI_VERSION = 660  # ssak_version() of the library this binding's struct layouts and signatures were written for


class GemmDesc(C.Structure):
    _fields_ = [("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("a_kmajor", C.c_int), ("b_kmajor", C.c_int),
                ("lda", C.c_long), ("ldb", C.c_long), ("ldc", C.c_long), ("nb1", C.c_int), ("nb2", C.c_int),
                ("sa1", C.c_long), ("sa2", C.c_long), ("sb1", C.c_long), ("sb2", C.c_long), ("sc1", C.c_long),
                ("sc2", C.c_long), ("alpha", C.c_float), ("epilogue", C.c_int), ("out_f32", C.c_int),
                ("accumulate", C.c_int), ("split_k", C.c_int), ("drop_p", C.c_float), ("drop_stream", C.c_uint32),
                ("drop_seed", C.c_uint64), ("bias_s2", C.c_long), ("pads_are_zero", C.c_int), ("colsum", C.c_int),
                ("dynamic_tiles", C.c_int), ("b_fragments", C.c_void_p), ("plan_tile", C.c_int)]


class W2V2Config(C.Structure):
    _fields_ = [("vocab_size", C.c_int), ("hidden_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int),
                ("intermediate_size", C.c_int), ("num_conv_layers", C.c_int), ("conv_dim", C.c_int * 8),
                ("conv_kernel", C.c_int * 8), ("conv_stride", C.c_int * 8), ("conv_bias", C.c_int),
                ("feat_extract_norm", C.c_int), ("do_stable_layer_norm", C.c_int),
                ("num_conv_pos_embeddings", C.c_int), ("num_conv_pos_embedding_groups", C.c_int),
                ("layer_norm_eps", C.c_float), ("attention_dropout", C.c_float), ("hidden_dropout", C.c_float),
                ("activation_dropout", C.c_float), ("feat_proj_dropout", C.c_float), ("final_dropout", C.c_float),
                ("freeze_feature_encoder", C.c_int), ("arch", C.c_int), ("num_mel_bins", C.c_int),
                ("max_source_positions", C.c_int), ("exact", C.c_int), ("adapter_attn_dim", C.c_int)]


class ProfEntry(C.Structure):
    _fields_ = [("name", C.c_char * 112), ("launches", C.c_long), ("total_ms", C.c_double), ("total_flops", C.c_double),
                ("bound", C.c_int)]


class NgramLMDesc(C.Structure):  # ssak_ngram_lm
    _fields_ = [("order", C.c_int), ("n_words", C.c_int), ("bos", C.c_int), ("eos", C.c_int), ("unk", C.c_int),
                ("trie_cap", C.c_int), ("n_nodes", C.c_int), ("trie", C.c_void_p), ("node_word", C.c_void_p), ("uni", C.c_void_p),
                ("ng_keys", C.c_void_p * 6), ("ng_val", C.c_void_p * 6), ("ng_cap", C.c_int * 6)]


class LMBeamParams(C.Structure):  # ssak_lm_beam_params
    _fields_ = [("beam_width", C.c_int), ("n_labels", C.c_int), ("blank", C.c_int), ("label_class", C.c_void_p),
                ("alpha", C.c_float), ("beta", C.c_float), ("beam_prune_logp", C.c_float), ("token_min_logp", C.c_float),
                ("unk_score_offset", C.c_float)]


class AudioBank(C.Structure):  # ssak_audio_bank
    _fields_ = [("n", C.c_int), ("data", C.c_void_p), ("offset", C.c_void_p), ("length", C.c_void_p), ("offset_host", C.c_void_p),
                ("length_host", C.c_void_p)]


# columns of the augmentation table (ssak_hip.h SSAK_AUG_*)
AUG_NONE, AUG_GAIN, AUG_NOISE_MIX, AUG_REVERB = -1, 0, 1, 2
(AUG_KIND, AUG_GAIN_DB, AUG_GAIN_LIN, AUG_SNR_DB, AUG_SNR_AMP, AUG_NOISE, AUG_NOISE_START, AUG_RIR, AUG_RIR_PEAK, AUG_RATE,
 AUG_OUT_LEN) = range(11)
AUG_NCOL = 11
AUG_FIR_MAX_TAPS, AUG_FIR_TILE = 255, 2048  # SSAK_AUG_FIR_MAX_TAPS, SSAK_AUG_FIR_TILE

GRAD_READY_FN = C.CFUNCTYPE(None, C.c_long, C.c_long, C.c_void_p)


def _load():
    if not os.path.exists(_LIB_PATH):
        raise ImportError(f"{_LIB_PATH} is missing: build it with `make` (or __graft_entry__.build()); "
                          "ssak_amd has no CPU fallback")
    lib = C.CDLL(_LIB_PATH)
    vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    sig = {
        "ssak_version": (i32, []),
        "ssak_last_error": (C.c_char_p, []),
        "ssak_wave_normalize_workspace_bytes": (sz, [i32, i32]),
        "ssak_wave_normalize": (i32, [vp, vp, i32, i32, vp, vp, vp, sz, vp]),
        "ssak_logmel_table_floats": (sz, []),
        "ssak_logmel_init_tables": (i32, [vp]),
        "ssak_logmel_workspace_bytes": (sz, [i32, i32]),
        "ssak_logmel_whisper": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, i32, i32, vp, sz, vp]),
        "ssak_ctc_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "ssak_ctc_loss_fwd_bwd": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, sz, vp]),
        "ssak_ctc_greedy_decode": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "ssak_augment_gain_noise_workspace_bytes": (sz, [i32, i32]),
        "ssak_augment_gain_noise": (i32, [vp, vp, vp, i32, i32, vp, vp, C.POINTER(AudioBank), vp, vp, sz, vp]),
        "ssak_augment_reverb_workspace_bytes": (sz, [i32, i32, i32]),
        "ssak_augment_reverb": (i32, [vp, vp, vp, i32, i32, vp, vp, C.POINTER(AudioBank), vp, vp, sz, vp]),
        "ssak_augment_time_stretch_workspace_bytes": (sz, [i32, i32, i32]),
        "ssak_augment_time_stretch": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, sz, vp]),
        "ssak_augment_fir_drop": (i32, [vp, i32, i32, vp, i32, vp, vp, vp, i32, vp, vp]),
        "ssak_ctc_lm_beam_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "ssak_ctc_lm_beam_decode": (i32, [vp, vp, i32, i32, i32, C.POINTER(NgramLMDesc), C.POINTER(LMBeamParams), vp, vp, vp,
                                          vp, sz, vp]),
        "ssak_lm_query": (i32, [C.POINTER(NgramLMDesc), vp, vp, i32, vp, vp]),
        "ssak_read_ranges": (i32, [vp, vp, vp, vp, i32, i32]),
        "ssak_drop_file_cache": (i32, [vp, i32]),
        "ssak_pcm_to_mono_f32": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp]),
        "ssak_resample_plan": (i32, [i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "ssak_resample_table": (i32, [i32, i32, vp]),
        "ssak_resample_sinc": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, vp]),
        "ssak_ctc_wer_workspace_bytes": (sz, [i32, i32, i32]),
        "ssak_ctc_wer": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
        "ssak_ctc_align_workspace_bytes": (sz, [i32, i32]),
        "ssak_ctc_forced_align": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
        "ssak_ctc_align_batch_workspace_bytes": (sz, [i32, i32, i32]),
        "ssak_ctc_forced_align_batch": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
        "ssak_gemm_bf16": (i32, [C.POINTER(GemmDesc), vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "ssak_gemm_f32": (i32, [C.POINTER(GemmDesc), vp, vp, vp, vp, vp, vp, vp]),
        "ssak_gemm_bf16_grouped": (i32, [C.POINTER(GemmDesc), i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]),
        "ssak_gemm_fragment_b_bytes": (sz, [i32, i32]),
        "ssak_gemm_fragment_b": (i32, [vp, C.c_long, i32, i32, i32, vp, vp]),
        "ssak_gemm_fragment_b_batched": (i32, [i32, C.POINTER(vp), C.POINTER(C.c_long), C.POINTER(i32), C.POINTER(i32),
                                              C.POINTER(i32), C.POINTER(vp), vp]),
        "ssak_gemm_uses_fragments": (i32, [C.POINTER(GemmDesc)]),
        "ssak_conv0_workspace_bytes": (sz, [i32, i32, i32]),
        "ssak_conv0_gn_gelu": (i32, [vp, vp, vp, vp, vp, vp, sz, i32, i32, i32, vp]),
        "ssak_conv0_gn_gelu_raw": (i32, [vp, vp, vp, vp, vp, vp, sz, i32, i32, i32, vp]),
        "ssak_prof_enable": (i32, [vp, i32]),
        "ssak_prof_enable_slots": (i32, [vp, C.POINTER(C.c_int32), i32]),
        "ssak_prof_collect": (i32, [vp, C.POINTER(ProfEntry), i32]),
        "ssak_attention_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32, C.c_uint64, C.c_uint32, vp]),
        "ssak_attention_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, C.c_uint64, C.c_uint32, i32, vp]),
        "ssak_attention_bwd_bias_workspace_bytes": (sz, [i32, i32, i32]),
        "ssak_attention_bwd_bias": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, C.c_uint64, C.c_uint32, vp, sz, vp]),
        "ssak_grad_sumsq": (i32, [vp, C.c_long, vp, vp, sz, vp]),
        "ssak_adamw_step": (i32, [vp, vp, vp, vp, vp, C.c_long, vp, f32, f32, f32, f32, f32, f32, f32, i32, vp]),
        "ssak_w2v2_create": (i32, [C.POINTER(W2V2Config), C.POINTER(vp)]),
        "ssak_w2v2_destroy": (None, [vp]),
        "ssak_w2v2_num_params": (C.c_long, [vp]),
        "ssak_w2v2_num_trainable": (C.c_long, [vp]),
        "ssak_w2v2_param_count": (i32, [vp]),
        "ssak_w2v2_param_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(C.c_long), C.POINTER(C.c_long),
                                       C.POINTER(i32), C.POINTER(C.c_long)]),
        "ssak_w2v2_bind": (i32, [vp, vp, vp, vp]),
        "ssak_w2v2_sync_weights": (i32, [vp, i32, vp]),
        "ssak_w2v2_num_frames": (i32, [vp, i32]),
        "ssak_w2v2_workspace_bytes": (sz, [vp, i32, i32, i32]),
        "ssak_w2v2_forward": (i32, [vp, vp, vp, i32, i32, vp, vp, C.c_uint64, i32, vp, vp, vp, sz, vp]),
        "ssak_w2v2_backward": (i32, [vp, vp, vp, sz, vp]),
        "ssak_w2v2_set_grad_ready_callback": (i32, [vp, GRAD_READY_FN, vp]),
        "ssak_w2v2_set_param_event": (i32, [vp, vp, vp, vp]),
        "ssak_w2v2_set_option": (i32, [vp, i32, i32]),
        "ssak_w2v2_grad_ranges": (i32, [C.POINTER(W2V2Config), C.POINTER(C.c_long), C.POINTER(C.c_long), i32]),
        "ssak_w2v2_forward_hidden": (i32, [vp, vp, vp, i32, i32, vp, vp, C.c_uint64, i32, vp, vp, vp, sz, vp]),
        "ssak_w2v2_backward_hidden": (i32, [vp, vp, vp, sz, vp]),
        "ssak_grad_sumsq_add": (i32, [vp, C.c_long, vp, vp, sz, vp]),
        "ssak_utt_norm_workspace_bytes": (sz, [i32]),
        "ssak_utt_norm_fwd": (i32, [vp, vp, i32, C.c_long, i32, f32, vp, vp, sz, vp]),
        "ssak_utt_norm_bwd": (i32, [vp, vp, vp, i32, C.c_long, i32, vp, vp, sz, vp]),
        "ssak_batchnorm_workspace_bytes": (sz, [i32]),
        "ssak_batchnorm_act_fwd": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, f32, f32, i32, f32, f32, C.c_uint64, C.c_uint32, vp, vp,
                                         vp, vp, sz, vp]),
        "ssak_batchnorm_act_bwd": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, f32, f32, C.c_uint64, C.c_uint32, vp, vp, vp, vp,
                                         vp, sz, vp]),
        "ssak_batchnorm_stats": (i32, [vp, i32, i32, vp, vp, sz, vp]),
        "ssak_adadelta_step": (i32, [vp, vp, vp, vp, vp, C.c_long, vp, f32, f32, f32, f32, f32, f32, vp]),
        "ssak_cast_f32_bf16": (i32, [vp, vp, C.c_long, vp]),
        "ssak_cast_bf16_f32": (i32, [vp, vp, C.c_long, vp]),
        "ssak_colsum_workspace_bytes": (sz, [i32]),
        "ssak_colsum_bf16": (i32, [vp, C.c_long, i32, i32, vp, vp, sz, vp]),
        "ssak_comm_unique_id": (i32, [vp]),
        "ssak_comm_create": (i32, [C.POINTER(vp), i32, i32, vp]),
        "ssak_allreduce": (i32, [vp, vp, C.c_long, C.c_long, i32, vp]),
        "ssak_comm_destroy": (i32, [vp]),
        "ssak_pool_fwd": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]),
        "ssak_pool_bwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
        "ssak_cls_head_fwd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, f32, C.c_uint64, i32, vp, vp, vp]),
        "ssak_cls_head_bwd_workspace_bytes": (sz, [i32, i32, i32]),
        "ssak_cls_head_bwd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, f32, C.c_uint64, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
        "ssak_cls_softmax_ce": (i32, [vp, vp, vp, i32, i32, f32, vp, vp, vp, vp]),
        "ssak_dec_embed": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
        "ssak_dec_attention_fwd": (i32, [vp, C.c_long, vp, C.c_long, vp, C.c_long, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
        "ssak_token_logprobs": (i32, [vp, i32, i32, i32, C.c_long, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "ssak_dec_attention_step_workspace_bytes": (sz, [i32, i32, i32]),
        "ssak_dec_attention_step": (i32, [vp, C.c_long, vp, C.c_long, C.c_long, vp, C.c_long, C.c_long, i32, vp, i32, i32, i32, i32, vp, sz, vp, vp]),
        "ssak_dec_greedy_step": (i32, [vp, C.c_long, i32, i32, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.c_long, i32, vp, vp]),
        "ssak_dec_timestamp_step": (i32, [vp, C.c_long, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.c_long,
                                          i32, vp, vp, vp]),
        "ssak_dec_sample_step": (i32, [vp, C.c_long, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.c_long,
                                       i32, vp, vp, f32, C.c_uint64, vp]),
        "ssak_dec_beam_topk": (i32, [vp, C.c_long, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, C.c_long, i32, vp, vp, i32, vp, vp, vp]),
        "ssak_dec_beam_select": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, C.c_long, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32,
                                       i32, i32, i32, i32, vp, vp]),
        "ssak_dec_kv_reorder": (i32, [vp, vp, i32, i32, i32, i32, i32, C.c_long, C.c_long, C.c_long, i32, i32, vp]),
        "ssak_dec_attention_step_grouped": (i32, [vp, C.c_long, vp, C.c_long, C.c_long, vp, C.c_long, C.c_long, i32, vp, i32, i32, i32, i32, i32, vp,
                                                  sz, vp, vp]),
        "ssak_layernorm_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, f32, i32, vp]),
        "ssak_dec_attention_fwd_lse": (i32, [vp, C.c_long, vp, C.c_long, vp, C.c_long, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
        "ssak_dec_attention_bwd": (i32, [vp, C.c_long, vp, C.c_long, vp, C.c_long, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp,
                                         C.c_long, vp, C.c_long, vp, C.c_long, vp, vp]),
        "ssak_dec_ce_bwd": (i32, [vp, i32, i32, C.c_long, vp, vp, f32, vp, C.c_long, vp, vp, vp]),
        "ssak_dec_embed_bwd": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]),
        "ssak_layernorm_fwd_stats": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, i32, vp]),
        "ssak_layernorm_bwd_workspace_bytes": (sz, [i32]),
        "ssak_layernorm_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, sz, vp]),
        "ssak_lora_fwd": (i32, [vp, C.c_long, vp, vp, vp, C.c_long, vp, i32, i32, i32, i32, f32, C.c_uint64, C.c_uint32, f32, vp]),
        "ssak_lora_bwd_input": (i32, [vp, C.c_long, vp, vp, vp, vp, C.c_long, i32, i32, i32, i32, i32, f32, C.c_uint64, C.c_uint32, f32, vp]),
        "ssak_lora_bwd_weights_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "ssak_lora_bwd_weights": (i32, [vp, C.c_long, vp, vp, vp, C.c_long, vp, vp, i32, i32, i32, i32, f32, C.c_uint64, C.c_uint32, f32, vp, sz, vp]),
        "ssak_lora_merge": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, f32, vp]),
        "ssak_debug_dropout_mask": (i32, [C.c_uint64, C.c_uint32, f32, C.c_long, i32, vp, C.POINTER(f32), vp]),
        "ssak_debug_attention_dropout_mask": (i32, [C.c_uint64, C.c_uint32, f32, i32, i32, i32, vp, vp]),
        "ssak_debug_layernorm_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, C.c_uint64, C.c_uint32, f32, C.c_uint32,
                                            f32, C.c_uint32, f32, i32, i32, vp]),
        "ssak_debug_layernorm_bwd_workspace_bytes": (sz, [i32]),
        "ssak_debug_layernorm_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, C.c_uint64, C.c_uint32, f32,
                                            C.c_uint32, f32, C.c_uint32, f32, i32, i32, vp, sz, vp]),
        "ssak_debug_softmax_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, C.c_uint64, C.c_uint32, f32, i32, vp]),
        "ssak_debug_softmax_bwd": (i32, [vp, vp, vp, i32, i32, i32, C.c_uint64, C.c_uint32, f32, i32, vp]),
        "ssak_debug_gelu": (i32, [vp, C.c_long, vp, vp, i32, vp]),
        "ssak_test_attn_adapter_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, i32, vp]),
        "ssak_debug_posconv_prepare": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        "ssak_debug_posconv_pack": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp]),
        "ssak_debug_posconv_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
        "ssak_debug_posconv_direct": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
        "ssak_debug_posconv_wgrad": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
        "ssak_debug_posconv_weight_bwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
        "ssak_debug_conv0_bwd_workspace_bytes": (sz, [i32, i32, i32]),
        "ssak_debug_conv0_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
        "ssak_debug_conv0_wgrad_workspace_bytes": (sz, [i32, i32, i32]),
        "ssak_debug_conv0_wgrad": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
        "ssak_debug_conv0_bias": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        "ssak_debug_col2im": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
        "ssak_debug_sum_slabs": (i32, [vp, i32, C.c_long, vp, vp]),
        "ssak_debug_conv_weight_rearrange": (i32, [vp, vp, i32, i32, i32, i32, vp]),
        "ssak_debug_conv_wgrad_unrearrange": (i32, [vp, vp, i32, i32, i32, vp]),
        "ssak_debug_col2im_k3s2": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
        "ssak_debug_mel_to_cl": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp]),
        "ssak_debug_add_rowvec": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
        "ssak_debug_copy_rows_padded": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
        "ssak_debug_specaug_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        "ssak_debug_specaug_bwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
        "ssak_debug_colsum": (i32, [vp, C.c_long, i32, i32, vp, vp, sz, vp, vp, i32, i32, vp]),
        "ssak_debug_gelu_grad_mul": (i32, [vp, vp, vp, C.c_long, i32, vp]),
        "ssak_debug_add": (i32, [vp, vp, vp, C.c_long, i32, vp]),
        "ssak_debug_transpose_batched": (i32, [i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), vp]),
        "ssak_debug_reduce": (i32, [i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_long), C.POINTER(i32), C.POINTER(i32), i32,
                                     C.POINTER(i32), i32, C.POINTER(i32), C.POINTER(i32), vp]),
    }
    lib.ssak_version.restype = i32
    got = lib.ssak_version()
    if got != ABI_VERSION:
        # struct layouts (GemmDesc, W2V2Config, ProfEntry) and signatures belong to ONE ABI: driving another build through
        # this table would pass arguments at the wrong offsets, so refuse it instead of skipping what it lacks
        raise ImportError(f"{_LIB_PATH} reports ABI {got}, this binding is written for {ABI_VERSION}: rebuild with `make`"
                          + (" (SSAK_HIP_LIB must name a build of the same ABI)" if os.environ.get("SSAK_HIP_LIB") else ""))
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


lib = _load()
SSAK_OK, SSAK_ERR_INVALID, SSAK_ERR_LAUNCH, SSAK_ERR_STATE = 0, -1, -2, -3
EPI_NONE, EPI_GELU, EPI_MUL_GELU_GRAD, EPI_GELU_SAVE_GRAD, EPI_MUL_AUX = 0, 1, 2, 3, 4
REDUCTION = {"sum": 0, "mean": 1}


def check(rc: int):
    if rc == SSAK_OK:
        return
    msg = lib.ssak_last_error().decode()
    if rc == SSAK_ERR_INVALID:
        raise ValueError(msg)
    if rc == SSAK_ERR_STATE:
        raise RuntimeError(msg)
    raise RuntimeError(f"libssak_hip status {rc}: {msg}")


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws(nbytes: int, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------ op wrappers (tensors in, tensors out)
def wave_normalize(x: torch.Tensor, lens: torch.Tensor | None = None, return_mask: bool = False):
    """[B,T] fp32 raw samples -> normalised [B,T] fp32 (+ int32 attention mask)."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    B, T = x.shape
    out = torch.empty_like(x)
    mask = torch.empty((B, T), dtype=torch.int32, device=x.device) if return_mask else None
    if lens is not None:
        lens = lens.to(device=x.device, dtype=torch.int32).contiguous()
    ws = _ws(lib.ssak_wave_normalize_workspace_bytes(B, T), x.device)
    check(lib.ssak_wave_normalize(ptr(x), ptr(lens), B, T, ptr(out), ptr(mask), ptr(ws), ws.numel(), stream()))
    return (out, mask) if return_mask else out


_LOGMEL_TABLES = {}


def logmel_tables(device):
    key = str(device)
    if key not in _LOGMEL_TABLES:
        t = torch.empty(lib.ssak_logmel_table_floats(), dtype=torch.float32, device=device)
        check(lib.ssak_logmel_init_tables(ptr(t)))
        _LOGMEL_TABLES[key] = t
    return _LOGMEL_TABLES[key]


def logmel_whisper(wav: torch.Tensor, lens: torch.Tensor | None = None, n_samples: int = 480000,
                   channels_last: torch.Tensor | None = None, cl_lead: int = 0, want_mel: bool = True):
    """[B,T] fp32 waveforms -> Whisper input features [B, 80, n_samples/160] fp32 (30 s windows by default)."""
    assert wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 2 and wav.is_contiguous()
    B, T = wav.shape
    if lens is not None:
        lens = lens.to(device=wav.device, dtype=torch.int32).contiguous()
    mel = torch.empty((B, 80, n_samples // 160), dtype=torch.float32, device=wav.device) if want_mel else None
    ws = _ws(lib.ssak_logmel_workspace_bytes(B, n_samples), wav.device)
    cl_rows = 0 if channels_last is None else channels_last.shape[1]
    check(lib.ssak_logmel_whisper(ptr(wav), ptr(lens), B, T, n_samples, ptr(logmel_tables(wav.device)), ptr(mel),
                                  ptr(channels_last), cl_rows, cl_lead, ptr(ws), ws.numel(), stream()))
    return mel


def ctc_loss(logits: torch.Tensor, in_lens: torch.Tensor | None, labels: torch.Tensor, blank: int = 0,
             reduction: str = "mean", zero_infinity: bool = True, grad_scale: float = 1.0, want_grad: bool = True):
    """logits [B,F,V] fp32, labels [B,L] (negative = pad) -> (loss[1], nll[B], dlogits[B,F,V] | None)."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3 and logits.is_contiguous()
    B, F, V = logits.shape
    if not labels.is_cuda and labels.numel() and int(labels.max()) >= V:
        raise ValueError(f"Label values must be <= vocab_size: {V}")  # modeling_wav2vec2.py:1686-1687
    # device-resident labels are validated by the kernel instead (bad label -> NaN nll): no host sync per step
    labels = labels.to(device=logits.device, dtype=torch.int32).contiguous()
    Lmax = labels.shape[1]
    if in_lens is not None:
        in_lens = in_lens.to(device=logits.device, dtype=torch.int32).contiguous()
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    nll = torch.empty(B, dtype=torch.float32, device=logits.device)
    grad = torch.empty_like(logits) if want_grad else None
    ws = _ws(lib.ssak_ctc_workspace_bytes(B, F, V, Lmax), logits.device)
    check(lib.ssak_ctc_loss_fwd_bwd(ptr(logits), ptr(in_lens), ptr(labels), B, F, V, Lmax, blank, REDUCTION[reduction],
                                    int(zero_infinity), float(grad_scale), ptr(loss), ptr(nll), ptr(grad), ptr(ws),
                                    ws.numel(), stream()))
    return loss, nll, grad


def ctc_greedy_decode(logits: torch.Tensor, in_lens: torch.Tensor | None = None, blank: int = 0):
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3 and logits.is_contiguous()
    B, F, V = logits.shape
    if in_lens is not None:
        in_lens = in_lens.to(device=logits.device, dtype=torch.int32).contiguous()
    ids = torch.empty((B, F), dtype=torch.int32, device=logits.device)
    n = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(lib.ssak_ctc_greedy_decode(ptr(logits), ptr(in_lens), B, F, V, blank, ptr(ids), ptr(n), stream()))
    return ids, n


def ctc_lm_beam_decode(logits: torch.Tensor, in_lens: torch.Tensor | None, lm: NgramLMDesc, *, n_labels: int, blank: int,
                       label_class: torch.Tensor, alpha: float, beta: float, beam_width: int, beam_prune_logp: float,
                       token_min_logp: float, unk_score_offset: float, workspace: torch.Tensor | None = None):
    """CTC beam search with an n-gram LM (``ssak_ctc_lm_beam_decode``; contract: ssak_amd/lm.py) -> (ids [B,F], n [B], score [B])."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3 and logits.is_contiguous()
    B, F, V = logits.shape
    if in_lens is not None:
        in_lens = in_lens.to(device=logits.device, dtype=torch.int32).contiguous()
    p = LMBeamParams(int(beam_width), int(n_labels), int(blank), label_class.data_ptr(), float(alpha), float(beta),
                     float(beam_prune_logp), float(token_min_logp), float(unk_score_offset))
    ids = torch.empty((B, F), dtype=torch.int32, device=logits.device)
    n = torch.empty(B, dtype=torch.int32, device=logits.device)
    score = torch.empty(B, dtype=torch.float32, device=logits.device)
    ws = workspace if workspace is not None else _ws(lib.ssak_ctc_lm_beam_workspace_bytes(B, F, V, int(beam_width)), logits.device)
    check(lib.ssak_ctc_lm_beam_decode(ptr(logits), ptr(in_lens), B, F, V, C.byref(lm), C.byref(p), ptr(ids), ptr(n), ptr(score),
                                      ptr(ws), ws.numel(), stream()))
    return ids, n, score


def _aug_args(x, lens, lens_host, params, params_host):
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    lens_host = np.ascontiguousarray(lens_host, dtype=np.int32)
    params_host = np.ascontiguousarray(params_host, dtype=np.float64)
    assert lens_host.shape == (x.shape[0],) and params_host.shape == (x.shape[0], AUG_NCOL)
    lens = lens.to(device=x.device, dtype=torch.int32).contiguous()
    params = params.to(device=x.device, dtype=torch.float64).contiguous()
    return lens, lens_host, params, params_host


def _hp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def augment_gain_noise(x, lens, lens_host, params, params_host, noise: AudioBank | None, out=None, workspace=None):
    """Gain / background-noise rows of the table applied to x [B,T] (``ssak_augment_gain_noise``; other rows copied) -> y [B,T]."""
    lens, lens_host, params, params_host = _aug_args(x, lens, lens_host, params, params_host)
    B, T = x.shape
    y = torch.empty_like(x) if out is None else out
    ws = workspace if workspace is not None else _ws(lib.ssak_augment_gain_noise_workspace_bytes(B, T), x.device)
    check(lib.ssak_augment_gain_noise(ptr(x), ptr(lens), _hp(lens_host), B, T, ptr(params), _hp(params_host),
                                      None if noise is None else C.byref(noise), ptr(y), ptr(ws), ws.numel(), stream()))
    return y


def augment_reverb(x, lens, lens_host, params, params_host, rirs: AudioBank | None, max_rir_len: int, out=None, workspace=None):
    """Reverberation rows of the table applied to x [B,T] (``ssak_augment_reverb``; other rows copied) -> y [B,T]."""
    lens, lens_host, params, params_host = _aug_args(x, lens, lens_host, params, params_host)
    B, T = x.shape
    y = torch.empty_like(x) if out is None else out
    ws = workspace if workspace is not None else _ws(lib.ssak_augment_reverb_workspace_bytes(B, T, max(1, int(max_rir_len))), x.device)
    check(lib.ssak_augment_reverb(ptr(x), ptr(lens), _hp(lens_host), B, T, ptr(params), _hp(params_host),
                                  None if rirs is None else C.byref(rirs), ptr(y), ptr(ws), ws.numel(), stream()))
    return y


def augment_time_stretch(x, lens, lens_host, params, params_host, T_out: int, workspace=None):
    """Time stretch of every row (``ssak_augment_time_stretch``) -> (y [B, T_out], out_lens [B] int32)."""
    lens, lens_host, params, params_host = _aug_args(x, lens, lens_host, params, params_host)
    B, T = x.shape
    y = torch.empty((B, int(T_out)), dtype=torch.float32, device=x.device)
    out_lens = torch.empty(B, dtype=torch.int32, device=x.device)
    ws = workspace if workspace is not None else _ws(lib.ssak_augment_time_stretch_workspace_bytes(B, T, int(T_out)), x.device)
    check(lib.ssak_augment_time_stretch(ptr(x), ptr(lens), _hp(lens_host), B, T, ptr(params), _hp(params_host), ptr(y), ptr(out_lens),
                                        int(T_out), ptr(ws), ws.numel(), stream()))
    return y, out_lens


def augment_fir_drop(x, taps=None, chunks=None, chunk_counts=None, chunk_counts_host=None, out=None):
    """``ssak_augment_fir_drop``: x [B,T] fp32 cross-correlated with ``taps`` [ntaps] (device fp32, odd length; None: no filter), the
    samples of ``chunks`` [B, max_chunks, 2] int32 (start, end; ``chunk_counts`` [B] int32 of them per row, on the device and,
    ``chunk_counts_host``, as a host array) set to 0 -> out [B,T], which must not be x."""
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    B, T = x.shape
    out = torch.empty_like(x) if out is None else out
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape
    ntaps = 0
    if taps is not None:
        assert taps.dtype == torch.float32 and taps.is_contiguous() and taps.dim() == 1
        ntaps = taps.numel()
    max_chunks, counts_h = 0, None
    if chunks is not None:
        assert chunks.dtype == torch.int32 and chunks.is_contiguous() and chunks.dim() == 3 and chunks.shape[0] == B and chunks.shape[2] == 2
        assert chunk_counts.dtype == torch.int32 and chunk_counts.is_contiguous() and chunk_counts.shape == (B,)
        counts_h = np.ascontiguousarray(chunk_counts_host, dtype=np.int32)
        assert counts_h.shape == (B,)
        max_chunks = chunks.shape[1]
    check(lib.ssak_augment_fir_drop(ptr(x), B, T, ptr(taps), ntaps, ptr(chunks), ptr(chunk_counts), None if counts_h is None else _hp(counts_h),
                                    max_chunks, ptr(out), stream()))
    return out


def lm_query(lm: NgramLMDesc, ctx_ids: torch.Tensor | None, words: torch.Tensor):
    """log10 P(words[q] | ctx_ids[q]) with ARPA backoff (``ssak_lm_query``); ctx_ids [Q, order-1] int32, most recent last
    (None for an order-1 LM, which has no context)."""
    words = words.to(dtype=torch.int32).contiguous()
    if ctx_ids is not None:
        ctx_ids = ctx_ids.to(device=words.device, dtype=torch.int32).contiguous()
    out = torch.empty(words.numel(), dtype=torch.float32, device=words.device)
    check(lib.ssak_lm_query(C.byref(lm), ptr(ctx_ids), ptr(words), words.numel(), ptr(out), stream()))
    return out


def ctc_wer(hyp_ids: torch.Tensor, hyp_lens: torch.Tensor, labels: torch.Tensor, token_class: torch.Tensor):
    """(edits [B], ref_words [B]) int32 on the device; see ``ssak_ctc_wer`` in include/ssak_hip.h."""
    B, F = hyp_ids.shape
    labels = labels.to(device=hyp_ids.device, dtype=torch.int32).contiguous()
    token_class = token_class.to(device=hyp_ids.device, dtype=torch.uint8).contiguous()
    Lmax, V = labels.shape[1], token_class.numel()
    edits = torch.empty(B, dtype=torch.int32, device=hyp_ids.device)
    nref = torch.empty(B, dtype=torch.int32, device=hyp_ids.device)
    ws = _ws(lib.ssak_ctc_wer_workspace_bytes(B, F, Lmax), hyp_ids.device)
    check(lib.ssak_ctc_wer(ptr(hyp_ids), ptr(hyp_lens), ptr(labels), ptr(token_class), B, F, Lmax, V, ptr(edits), ptr(nref),
                           ptr(ws), ws.numel(), stream()))
    return edits, nref


def gemm(A, B, C_out, M, N, K, *, a_kmajor=False, b_kmajor=False, lda=None, ldb=None, ldc=None, nb1=1, nb2=1,
         sa=(0, 0), sb=(0, 0), sc=(0, 0), alpha=1.0, bias=None, epilogue=EPI_NONE, aux_in=None, aux_out=None,
         accumulate=False, split_k=1, drop_p=0.0, drop_stream=0, drop_seed=0, pads_are_zero=False, colsum_out=None,
         dynamic_tiles=False, b_fragments=None, plan_tile=0):
    """Raw descriptor-level GEMM on device tensors (see ``ssak_gemm_desc`` in include/ssak_hip.h).  ``b_fragments``: the
    copy of B made by :func:`gemm_fragment_b` (used when the library picks the B-direct kernel, ignored otherwise)."""
    d = GemmDesc(M, N, K, int(a_kmajor), int(b_kmajor), lda, ldb, ldc, nb1, nb2, sa[0], sa[1], sb[0], sb[1], sc[0],
                 sc[1], float(alpha), epilogue, int(C_out.dtype == torch.float32), int(accumulate), split_k, float(drop_p),
                 drop_stream, drop_seed, 0, int(pads_are_zero), int(colsum_out is not None), int(dynamic_tiles),
                 ptr(b_fragments), int(plan_tile))
    n_slabs = split_k if split_k > 0 else max(1, min(32, ((K + 63) // 64) // 4))  # 0 = library-sized split
    ws = _ws(n_slabs * nb1 * nb2 * M * N * 4, A.device) if n_slabs > 1 else None
    if colsum_out is not None:
        aux_out = colsum_out
        ws = _ws(((M + 63) // 64) * N * 4, A.device)
    check(lib.ssak_gemm_bf16(C.byref(d), ptr(A), ptr(B), ptr(C_out), ptr(bias), ptr(aux_in), ptr(aux_out), ptr(ws),
                             0 if ws is None else ws.numel(), stream()))
    return C_out


def gemm_fragment_b(B, N, K, *, ldb=None, b_kmajor=False):
    """Fragment-ordered copy of a weight operand (``ssak_gemm_fragment_b``): a bf16 tensor of ``ssak_gemm_fragment_b_bytes``."""
    ldb = ldb if ldb is not None else (N if b_kmajor else K)
    out = torch.empty(lib.ssak_gemm_fragment_b_bytes(N, K) // 2, dtype=torch.bfloat16, device=B.device)
    check(lib.ssak_gemm_fragment_b(ptr(B), ldb, N, K, int(b_kmajor), ptr(out), stream()))
    return out


def gemm_uses_fragments(M, N, K, *, a_kmajor=False, b_kmajor=False, lda=None, ldb=None, ldc=None, pads_are_zero=False):
    d = GemmDesc(M, N, K, int(a_kmajor), int(b_kmajor), lda if lda is not None else (M if a_kmajor else K),
                 ldb if ldb is not None else (N if b_kmajor else K), ldc if ldc is not None else N, 1, 1, 0, 0, 0, 0, 0, 0, 1.0,
                 EPI_NONE, 0, 0, 1, 0.0, 0, 0, 0, int(pads_are_zero), 0, 0, None)
    return bool(lib.ssak_gemm_uses_fragments(C.byref(d)))


def gemm_f32(A, B, C_out, M, N, K, *, a_kmajor=False, b_kmajor=False, lda=None, ldb=None, ldc=None, nb1=1, nb2=1,
             sa=(0, 0), sb=(0, 0), sc=(0, 0), alpha=1.0, bias=None, epilogue=EPI_NONE, aux_in=None, aux_out=None,
             accumulate=False, drop_p=0.0, drop_stream=0, drop_seed=0, colsum_out=None, bias_s2=0):
    """The fp32 GEMM of the exact mode (``ssak_gemm_f32``): same descriptor as :func:`gemm`, float tensors."""
    d = GemmDesc(M, N, K, int(a_kmajor), int(b_kmajor), lda, ldb, ldc, nb1, nb2, sa[0], sa[1], sb[0], sb[1], sc[0],
                 sc[1], float(alpha), epilogue, 1, int(accumulate), 1, float(drop_p), drop_stream, drop_seed, bias_s2, 0,
                 int(colsum_out is not None), 0)
    if colsum_out is not None:
        aux_out = colsum_out
    check(lib.ssak_gemm_f32(C.byref(d), ptr(A), ptr(B), ptr(C_out), ptr(bias), ptr(aux_in), ptr(aux_out), stream()))
    return C_out


def gemm_grouped(problems, stream_=None, dynamic_tiles=False):
    """problems: list of (A, B, C_out, M, N, K, lda, ldb, ldc) sharing K / layouts (a_kmajor, b_kmajor passed per call via
    keyword in each tuple's dict is not needed: the weight-gradient form is k-major on both operands)."""
    n = len(problems)
    descs = (GemmDesc * n)()
    pa, pb, pc = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    for i, (A, B, Cout, M, N, K, lda, ldb, ldc, akm, bkm) in enumerate(problems):
        descs[i] = GemmDesc(M, N, K, int(akm), int(bkm), lda, ldb, ldc, 1, 1, 0, 0, 0, 0, 0, 0, 1.0, 0,
                            int(Cout.dtype == torch.float32), 0, 1, 0.0, 0, 0, 0, 1, 0, int(dynamic_tiles))
        pa[i], pb[i], pc[i] = A.data_ptr(), B.data_ptr(), Cout.data_ptr()
    check(lib.ssak_gemm_bf16_grouped(descs, n, pa, pb, pc, stream()))


DTYPE_F32, DTYPE_BF16 = 0, 1


class Comm:
    """RCCL communicator behind the C ABI (``ssak_comm_*`` / ``ssak_allreduce``): what a host without torch.distributed uses for
    the data-parallel exchange.  ``unique_id()`` on rank 0, the 128 bytes carried to the other ranks by the host's own means,
    then ``Comm(world, rank, id)`` on every rank (collective)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        check(lib.ssak_comm_unique_id(buf))
        return buf.raw

    def __init__(self, world: int, rank: int, uid: bytes):
        assert len(uid) == 128
        self._h = C.c_void_p()
        check(lib.ssak_comm_create(C.byref(self._h), int(world), int(rank), C.create_string_buffer(uid, 128)))
        self.world, self.rank = world, rank

    def all_reduce(self, t: torch.Tensor, offset: int = 0, count: int | None = None, stream_=None):
        """In-place sum over ranks of ``t.view(-1)[offset : offset + count]`` (fp32 or bf16), asynchronous on the current stream."""
        dt = {torch.float32: DTYPE_F32, torch.bfloat16: DTYPE_BF16}[t.dtype]
        n = t.numel() - offset if count is None else count
        check(lib.ssak_allreduce(self._h, ptr(t), int(offset), int(n), dt, stream() if stream_ is None else stream_))

    def close(self):
        if self._h:
            check(lib.ssak_comm_destroy(self._h))
            self._h = C.c_void_p()


def prof_enable(mode: int):
    """Launch timing on the CURRENT stream: 0 = off, 1 = every launch, 2 + i = only the slot at index i of
    :func:`prof_collect`'s list.  Per stream: other streams / handles are neither slowed nor recorded."""
    check(lib.ssak_prof_enable(stream(), int(mode)))


def prof_enable_slots(slots):
    """Launch timing on the CURRENT stream for the slots at these indices of :func:`prof_collect`'s list only."""
    arr = (C.c_int32 * len(slots))(*[int(v) for v in slots])
    check(lib.ssak_prof_enable_slots(stream(), arr, len(slots)))


BOUNDS = {0: "mfma", 1: "hbm", 2: "latency"}


def prof_collect():
    """[(kernel name, launches, total ms, total algorithmic work, bound)] since the last collect; work = flops for "mfma"
    slots, bytes for "hbm" / "latency" slots."""
    arr = (ProfEntry * 128)()
    n = lib.ssak_prof_collect(stream(), arr, 128)
    if n < 0:
        check(n)
    return [(arr[i].name.decode(), arr[i].launches, arr[i].total_ms, arr[i].total_flops, BOUNDS[arr[i].bound]) for i in range(n)]


def conv0_gn_gelu(x: torch.Tensor, w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, raw: bool = False):
    """x [B, T] fp32, w [C, 10], gamma / beta [C] -> [B, T0, C] bf16 (conv k=10 s=5 -> GroupNorm per channel -> GELU).  ``raw``:
    x are RAW full-length waveforms, the zero-mean / unit-variance normalisation folded into the GroupNorm statistics."""
    B, T = x.shape
    C = w.shape[0]
    T0 = (T - 10) // 5 + 1
    out = torch.full((B, T0, C), float("nan"), dtype=torch.bfloat16, device=x.device)
    nb = lib.ssak_conv0_workspace_bytes(B, T, C)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    fn = lib.ssak_conv0_gn_gelu_raw if raw else lib.ssak_conv0_gn_gelu
    check(fn(ptr(x), ptr(w.contiguous()), ptr(gamma), ptr(beta), ptr(out), ptr(ws), nb, B, T, C, stream()))
    return out


def attention_fwd(qkv: torch.Tensor, B: int, F: int, nh: int, klens=None, drop_p=0.0, seed=0, stream_id=0):
    """qkv [B*F, 3H] bf16 -> (ctx [B*F, H] bf16, lse [B, nh, F] fp32)."""
    H = qkv.shape[1] // 3
    ctx = torch.empty((B * F, H), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((B, nh, F), dtype=torch.float32, device=qkv.device)
    if klens is not None:
        klens = klens.to(device=qkv.device, dtype=torch.int32).contiguous()
    check(lib.ssak_attention_fwd(ptr(qkv), ptr(ctx), ptr(lse), ptr(klens), B, F, nh, H, float(drop_p), seed, stream_id, stream()))
    return ctx, lse


ATTN_BWD_DEFAULT, ATTN_BWD_TWO_KERNEL = 0, 1
W2V2_OPT_DYNAMIC_TILES, W2V2_OPT_ATTENTION_BWD, W2V2_OPT_POSCONV_DIRECT, W2V2_OPT_FRAGMENT_WEIGHTS, W2V2_OPT_TRANSPOSED_WEIGHTS = 1, 2, 3, 4, 5
W2V2_OPT_RAW_INPUT = 6


def attention_bwd(qkv, ctx, lse, dctx, B: int, F: int, nh: int, klens=None, drop_p=0.0, seed=0, stream_id=0,
                  mode=ATTN_BWD_DEFAULT):
    """``mode``: ATTN_BWD_DEFAULT = ATTN_BWD_TWO_KERNEL (dQ; dK + dV); the single-pass form (2) was removed in ABI 400."""
    H = qkv.shape[1] // 3
    dqkv = torch.full_like(qkv, float("nan"))  # poisoned: the kernels write every element
    delta = torch.empty((B, nh, F), dtype=torch.float32, device=qkv.device)
    if klens is not None:
        klens = klens.to(device=qkv.device, dtype=torch.int32).contiguous()
    check(lib.ssak_attention_bwd(ptr(qkv), ptr(ctx), ptr(lse), ptr(klens), ptr(dctx), ptr(delta), ptr(dqkv), B, F, nh, H,
                                 float(drop_p), seed, stream_id, int(mode), stream()))
    return dqkv


def attention_bwd_bias(qkv, ctx, lse, dctx, B: int, F: int, nh: int, klens=None, drop_p=0.0, seed=0, stream_id=0, bias_grad=None):
    """attention_bwd + the q|k|v projection bias gradient (column sums of dqkv, taken inside the kernels): ``bias_grad`` [3H] fp32
    is ADDED to (zeros when None).  Returns (dqkv, bias_grad)."""
    H = qkv.shape[1] // 3
    dqkv = torch.full_like(qkv, float("nan"))
    delta = torch.empty((B, nh, F), dtype=torch.float32, device=qkv.device)
    if bias_grad is None:
        bias_grad = torch.zeros(3 * H, dtype=torch.float32, device=qkv.device)
    if klens is not None:
        klens = klens.to(device=qkv.device, dtype=torch.int32).contiguous()
    nbytes = lib.ssak_attention_bwd_bias_workspace_bytes(B, F, H)
    ws = _ws(nbytes, qkv.device)
    check(lib.ssak_attention_bwd_bias(ptr(qkv), ptr(ctx), ptr(lse), ptr(klens), ptr(dctx), ptr(delta), ptr(dqkv), ptr(bias_grad), B, F,
                                      nh, H, float(drop_p), seed, stream_id, ptr(ws), nbytes, stream()))
    return dqkv, bias_grad


# ------------------------------------------------------------------ utterance classification (ABI 580): pooling, head, loss
POOL_MODES = {"mean": 0, "sum": 1, "max": 2}  # SSAK_POOL_*
CLS_SITE_INPUT, CLS_SITE_HIDDEN = 4, 5  # SSAK_CLS_SITE_*: the head's two dropout sites on its [B, H] tensors


def _host_i32(values, n: int, what: str):
    """The host mirror of a small int32 device vector (lengths, labels): the library validates it before any launch."""
    if torch.is_tensor(values):
        values = values.detach().cpu().numpy()
    a = np.ascontiguousarray(values, dtype=np.int32).reshape(-1)
    if a.shape != (n,):
        raise ValueError(f"{what}: expected {n} values, got {a.shape[0]}")
    return a


def pool_fwd(hidden: torch.Tensor, frame_lens=None, mode: str = "mean"):
    """hidden [B,F,H] bf16 (or fp32, the exact mode) -> (pooled [B,H] fp32, argmax [B,H] int32 | None) over the frames
    ``< frame_lens[b]`` (host values; None = all F frames, padding included).  ``ssak_pool_fwd``."""
    assert hidden.is_cuda and hidden.dim() == 3 and hidden.is_contiguous()
    B, F, H = hidden.shape
    lens_h = None if frame_lens is None else _host_i32(frame_lens, B, "frame_lens")
    lens_d = None if lens_h is None else torch.from_numpy(lens_h).to(hidden.device)
    pooled = torch.empty((B, H), dtype=torch.float32, device=hidden.device)
    argmax = torch.empty((B, H), dtype=torch.int32, device=hidden.device) if mode == "max" else None
    check(lib.ssak_pool_fwd(ptr(hidden), ptr(lens_d), _hp(lens_h), B, F, H, POOL_MODES[mode], _row_dtype(hidden), ptr(pooled), ptr(argmax),
                            stream()))
    return pooled, argmax


def pool_bwd(dpooled: torch.Tensor, argmax, frame_lens, F: int, mode: str = "mean", dtype: torch.dtype = torch.bfloat16):
    """d loss / d pooled [B,H] fp32 -> d loss / d hidden [B,F,H] of ``dtype``, every element written (``ssak_pool_bwd``)."""
    assert dpooled.is_cuda and dpooled.dtype == torch.float32 and dpooled.dim() == 2 and dpooled.is_contiguous()
    B, H = dpooled.shape
    lens_h = None if frame_lens is None else _host_i32(frame_lens, B, "frame_lens")
    lens_d = None if lens_h is None else torch.from_numpy(lens_h).to(dpooled.device)
    dhidden = torch.empty((B, int(F), H), dtype=dtype, device=dpooled.device)
    check(lib.ssak_pool_bwd(ptr(dpooled), ptr(argmax), ptr(lens_d), _hp(lens_h), B, int(F), H, POOL_MODES[mode], _row_dtype(dhidden),
                            ptr(dhidden), stream()))
    return dhidden


def cls_head_fwd(pooled, W1, b1, W2, b2, drop_p: float = 0.0, seed: int = 0, training: bool = False):
    """pooled [B,H] fp32 -> (logits [B,C], act [B,H] = tanh(dense(drop(pooled))), saved for the backward).  ``ssak_cls_head_fwd``."""
    B, H = pooled.shape
    Cn = W2.shape[0]
    act = torch.empty((B, H), dtype=torch.float32, device=pooled.device)
    logits = torch.empty((B, Cn), dtype=torch.float32, device=pooled.device)
    check(lib.ssak_cls_head_fwd(ptr(pooled), ptr(W1), ptr(b1), ptr(W2), ptr(b2), B, H, Cn, float(drop_p), C.c_uint64(int(seed)), int(bool(training)),
                                ptr(act), ptr(logits), stream()))
    return logits, act


def cls_head_bwd(dlogits, pooled, act, W1, W2, dW1, db1, dW2, db2, drop_p: float = 0.0, seed: int = 0, training: bool = False):
    """The head's backward into the caller's gradient tensors (overwritten) -> d loss / d pooled [B,H].  ``ssak_cls_head_bwd``."""
    B, H = pooled.shape
    Cn = W2.shape[0]
    dpooled = torch.empty_like(pooled)
    ws = _ws(lib.ssak_cls_head_bwd_workspace_bytes(B, H, Cn), pooled.device)
    check(lib.ssak_cls_head_bwd(ptr(dlogits), ptr(pooled), ptr(act), ptr(W1), ptr(W2), B, H, Cn, float(drop_p), C.c_uint64(int(seed)),
                                int(bool(training)), ptr(dW1), ptr(db1), ptr(dW2), ptr(db2), ptr(dpooled), ptr(ws), ws.numel(), stream()))
    return dpooled


def cls_softmax_ce(logits: torch.Tensor, labels=None, grad_scale: float = 1.0, want_grad: bool = True):
    """logits [B,C] fp32 -> (probs [B,C], loss [1] | None, dlogits [B,C] | None); ``labels`` are host values (or a tensor, read
    back once), validated by the library before the launch.  ``ssak_cls_softmax_ce``."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
    B, Cn = logits.shape
    probs = torch.empty_like(logits)
    lab_h = None if labels is None else _host_i32(labels, B, "labels")
    lab_d = None if lab_h is None else torch.from_numpy(lab_h).to(logits.device)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device) if lab_h is not None else None
    dlogits = torch.empty_like(logits) if lab_h is not None and want_grad else None
    check(lib.ssak_cls_softmax_ce(ptr(logits), ptr(lab_d), _hp(lab_h), B, Cn, float(grad_scale), ptr(probs), ptr(loss), ptr(dlogits), stream()))
    return probs, loss, dlogits


# ------------------------------------------------------------------ the Whisper text decoder (ABI 600)
DEC_HEAD_DIM = 64  # the head dimension of every Whisper size, the one ssak_dec_attention_fwd is built for


def dec_embed(embed_tokens: torch.Tensor, embed_positions: torch.Tensor, ids, pos_offset: int = 0, out=None):
    """ids [B, L] (host values, or a tensor read back once) -> [B * L, D] bf16 = embed_tokens[ids] + embed_positions[pos_offset + i]
    (``ssak_dec_embed``); a bad id or an overrun of the position table is a ``ValueError`` and launches nothing."""
    assert embed_tokens.is_cuda and embed_tokens.dtype == torch.bfloat16 and embed_tokens.is_contiguous()
    assert embed_positions.dtype == torch.bfloat16 and embed_positions.is_contiguous()
    ids_np = ids.detach().cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)
    B, L = ids_np.shape
    V, D = embed_tokens.shape
    ids_h = np.ascontiguousarray(ids_np, dtype=np.int32).reshape(-1)
    ids_d = torch.from_numpy(ids_h).to(embed_tokens.device)
    out = torch.empty((B * L, D), dtype=torch.bfloat16, device=embed_tokens.device) if out is None else out
    check(lib.ssak_dec_embed(ptr(embed_tokens), ptr(embed_positions), ptr(ids_d), _hp(ids_h), B, L, D, V, embed_positions.shape[0],
                             int(pos_offset), ptr(out), stream()))
    return out


def _dec_attention_fwd(q, k, v, B, Lq, Lk, nh, klens, causal, q_offset, head_dim, ctx, lse):
    """:func:`dec_attention_fwd` (``lse`` None) and :func:`dec_attention_fwd_lse`: one body, the entry with or without the lse output."""
    for t in (q, k, v):
        assert t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 2 and t.stride(1) == 1
    assert q.shape[0] == B * Lq and k.shape[0] == B * Lk and v.shape[0] == B * Lk, "q holds B * Lq rows, k and v B * Lk"
    kl_h = None if klens is None else _host_i32(klens, B, "klens")
    kl_d = None if kl_h is None else torch.from_numpy(kl_h).to(q.device)
    ctx = torch.empty((B * Lq, nh * head_dim), dtype=torch.bfloat16, device=q.device) if ctx is None else ctx
    assert ctx.dtype == torch.bfloat16 and ctx.is_contiguous() and ctx.shape == (B * Lq, nh * head_dim)
    args = (ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), int(Lk), ptr(kl_d), _hp(kl_h), B, int(Lq), int(nh), int(head_dim),
            int(bool(causal)), int(q_offset), ptr(ctx))
    if lse is None:
        check(lib.ssak_dec_attention_fwd(*args, stream()))
    else:
        assert lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() == B * nh * Lq
        check(lib.ssak_dec_attention_fwd_lse(*args, ptr(lse), stream()))
    return ctx, lse


def dec_attention_fwd(q, k, v, B: int, Lq: int, Lk: int, nh: int, *, klens=None, causal: bool = False, q_offset: int = 0,
                      head_dim: int = DEC_HEAD_DIM, ctx=None):
    """``ssak_dec_attention_fwd``: q [B * Lq, ldq], k / v [B * Lk, ldk / ldv] bf16 -- 2-D tensors or column slices of one (their row
    stride is passed on) -> ctx [B * Lq, nh * 64] bf16.  ``klens``: host values [B] (None: all Lk keys)."""
    return _dec_attention_fwd(q, k, v, B, Lq, Lk, nh, klens, causal, q_offset, head_dim, ctx, None)[0]


def token_logprobs(logits: torch.Tensor, V: int, targets=None, allowed=None):
    """``ssak_token_logprobs`` on logits [R, ldv] (fp32 or bf16, the first V columns valid) -> (lse [R], logprob [R] | None, argmax
    [R] int32, probs [R, n_allowed] | None).  ``targets`` [R] and ``allowed`` [n] are host values; a negative target is not scored."""
    assert logits.is_cuda and logits.dim() == 2 and logits.stride(1) == 1
    R, dev = logits.shape[0], logits.device
    tg_h = None if targets is None else _host_i32(targets, R, "targets")
    tg_d = None if tg_h is None else torch.from_numpy(tg_h).to(dev)
    al_h = None if allowed is None else np.ascontiguousarray(allowed, dtype=np.int32).reshape(-1)
    al_d = None if al_h is None else torch.from_numpy(al_h).to(dev)
    n_al = 0 if al_h is None else al_h.shape[0]
    lse = torch.empty(R, dtype=torch.float32, device=dev)
    logprob = torch.empty(R, dtype=torch.float32, device=dev) if tg_h is not None else None
    argmax = torch.empty(R, dtype=torch.int32, device=dev)
    probs = torch.empty((R, n_al), dtype=torch.float32, device=dev) if n_al else None
    check(lib.ssak_token_logprobs(ptr(logits), _row_dtype(logits), R, int(V), logits.stride(0), ptr(tg_d), _hp(tg_h), ptr(al_d), _hp(al_h), n_al,
                                  ptr(lse), ptr(logprob), ptr(argmax), ptr(probs), stream()))
    return lse, logprob, argmax, probs


# ------------------------------------------------------------------ Whisper generation (ABI 610, 620): no host copies, nothing read back
def dec_attention_step_workspace(B: int, nh: int, n_split: int = 0, device="cuda:0"):
    """The fp32 workspace of :func:`dec_attention_step` for ``n_split`` pieces (0: enough for any split the library chooses)."""
    return torch.empty(max(lib.ssak_dec_attention_step_workspace_bytes(int(B), int(nh), int(n_split)) // 4, 4), dtype=torch.float32, device=device)


def dec_attention_step(q, k, v, n_keys: int, nh: int, *, klens=None, n_split: int = 0, workspace=None, head_dim: int = DEC_HEAD_DIM, ctx=None):
    """:func:`dec_attention_step_grouped` with ``group = 1`` (all ``ssak_dec_attention_step`` does): q [B, ldq]; k / v [B, capacity,
    ld] bf16 views (row and per-utterance strides are passed on: a cache with spare capacity, column slices of a packed k|v
    buffer) -> ctx [B, nh * 64] bf16 over the keys ``< n_keys`` and ``< klens[b]``.  ``klens``: an int32 DEVICE tensor [B] the caller has validated (>= 1), or None.  ``n_split``: 0 = the library
    chooses.  ``workspace``: from :func:`dec_attention_step_workspace` (allocated per call when None)."""
    return dec_attention_step_grouped(q, k, v, n_keys, nh, 1, klens=klens, n_split=n_split, workspace=workspace, head_dim=head_dim, ctx=ctx)


def _assert_masks(V: int, *masks):
    for m in masks:
        assert m is None or (m.is_cuda and m.dtype == torch.uint8 and m.numel() == V and m.is_contiguous())


def _h_next_dims(embed_tokens, embed_positions, h_next, rows: int):
    """(D, max_positions) of the tables behind ``h_next`` [rows, D] bf16; (0, 0) when no ``h_next`` is formed."""
    if h_next is None:
        return 0, 0
    assert embed_tokens.dtype == torch.bfloat16 and embed_tokens.is_contiguous() and embed_positions.is_contiguous()
    D, max_pos = embed_tokens.shape[1], embed_positions.shape[0]
    assert h_next.dtype == torch.bfloat16 and h_next.is_contiguous() and tuple(h_next.shape) == (rows, D)
    return D, max_pos


def _token_step(entry, rules, tail, logits, V, finished, n_unfinished, tokens, logprobs, t, eos_id, pad_id, suppress, begin_suppress, first,
                embed_tokens, embed_positions, next_pos, h_next):
    """The one body of :func:`dec_greedy_step`, :func:`dec_timestamp_step` and :func:`dec_sample_step`: the checks, then ``entry`` with
    the arguments the three share, the timestamp ``rules`` (ts_begin, no_timestamps_id, max_initial, ts_last; None for the entry
    without them) and the entry's own ``tail``."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    B = logits.shape[0]
    assert tokens.dtype == torch.int32 and logprobs.dtype == torch.float32 and tokens.shape == logprobs.shape and tokens.shape[0] == B
    assert tokens.is_contiguous() and logprobs.is_contiguous()
    assert finished.dtype == torch.uint8 and finished.numel() == B and n_unfinished.dtype == torch.int32
    _assert_masks(V, suppress, begin_suppress)
    D, max_pos = _h_next_dims(embed_tokens, embed_positions, h_next, B)
    head = (ptr(logits), logits.stride(0), B, int(V), ptr(suppress), ptr(begin_suppress), int(bool(first)))
    mid = (ptr(embed_tokens), ptr(embed_positions), D, max_pos, int(next_pos), int(eos_id), int(pad_id), ptr(finished), ptr(n_unfinished),
           ptr(tokens), ptr(logprobs), tokens.shape[1], int(t))
    if rules is not None:
        ts_begin, no_timestamps_id, max_initial, ts_last = rules
        assert ts_last is None or (ts_last.is_cuda and ts_last.dtype == torch.int32 and ts_last.numel() == B and ts_last.is_contiguous())
        head += (int(ts_begin), int(no_timestamps_id), int(max_initial))
        mid += (ptr(ts_last),)
    check(entry(*head, *mid, ptr(h_next), *tail, stream()))


def dec_greedy_step(logits, V: int, *, finished, n_unfinished, tokens, logprobs, t: int, eos_id: int, pad_id: int, suppress=None,
                    begin_suppress=None, first: bool = False, embed_tokens=None, embed_positions=None, next_pos: int = 0, h_next=None):
    """``ssak_dec_greedy_step`` on logits [B, ldv] fp32: writes ``tokens[:, t]`` (int32 [B, ldt]), ``logprobs[:, t]`` (fp32, same
    shape), ``finished`` (uint8 [B], read and written), ``n_unfinished`` (int32 [1]) and, when ``h_next`` [B, D] bf16 is given,
    the next step's input row ``embed_tokens[token] + embed_positions[next_pos]``.  ``suppress`` / ``begin_suppress``: uint8 [V]
    device masks.  Everything stays on the device."""
    _token_step(lib.ssak_dec_greedy_step, None, (), logits, V, finished, n_unfinished, tokens, logprobs, t, eos_id, pad_id, suppress,
                begin_suppress, first, embed_tokens, embed_positions, next_pos, h_next)


def dec_timestamp_step(logits, V: int, *, finished, n_unfinished, tokens, logprobs, t: int, eos_id: int, pad_id: int, ts_begin: int,
                       no_timestamps_id: int, ts_last, max_initial: int = -1, suppress=None, begin_suppress=None, first: bool = False,
                       embed_tokens=None, embed_positions=None, next_pos: int = 0, h_next=None):
    """``ssak_dec_timestamp_step`` (ABI 620): :func:`dec_greedy_step` under whisper's timestamp rules.  ``ts_last``: int32 [B] on the
    device, the row's most recent timestamp id or -1 (written at ``t == 0``, read and updated afterwards); ``max_initial``: the
    largest index of the first timestamp, -1 for none.  The history is what the kernel wrote at ``tokens[:, :t]``."""
    _token_step(lib.ssak_dec_timestamp_step, (ts_begin, no_timestamps_id, max_initial, ts_last), (), logits, V, finished, n_unfinished, tokens,
                logprobs, t, eos_id, pad_id, suppress, begin_suppress, first, embed_tokens, embed_positions, next_pos, h_next)


def dec_sample_step(logits, V: int, *, finished, n_unfinished, tokens, logprobs, t: int, eos_id: int, pad_id: int, temperature: float, seed: int,
                    ts_begin: int = 0, no_timestamps_id: int = 0, ts_last=None, max_initial: int = -1, suppress=None, begin_suppress=None,
                    first: bool = False, embed_tokens=None, embed_positions=None, next_pos: int = 0, h_next=None):
    """``ssak_dec_sample_step`` (ABI 640): :func:`dec_timestamp_step` (``ts_last=None``: :func:`dec_greedy_step`, no rules) drawing the
    token from ``softmax(x / temperature)`` over the filtered row instead of taking its maximum; the log-probability is the drawn
    token's under the untempered row.  The draw is a function of ``(seed, t, row, column)``: the same call gives the same bits."""
    _token_step(lib.ssak_dec_sample_step, (ts_begin, no_timestamps_id, max_initial, ts_last), (float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF),
                logits, V, finished, n_unfinished, tokens, logprobs, t, eos_id, pad_id, suppress, begin_suppress, first, embed_tokens,
                embed_positions, next_pos, h_next)


# ------------------------------------------------------------------ Whisper beam search (ABI 630): nb hypotheses per audio, R = B * nb rows
def dec_attention_step_grouped(q, k, v, n_keys: int, nh: int, group: int, *, klens=None, n_split: int = 0, workspace=None,
                               head_dim: int = DEC_HEAD_DIM, ctx=None):
    """``ssak_dec_attention_step_grouped``: :func:`dec_attention_step` where query row ``r`` of q [R, ldq] reads k / v [R / group,
    capacity, ld] of utterance ``r // group`` and ``klens[r // group]``: the beams of an audio share one cross k|v buffer."""
    assert q.is_cuda and q.dtype == torch.bfloat16 and q.dim() == 2 and q.stride(1) == 1
    R, group = q.shape[0], int(group)
    for t in (k, v):
        assert t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 3 and t.stride(2) == 1
        assert group < 1 or R % group or t.shape[0] == R // group  # (a group that does not divide the rows is the library's refusal)
    assert klens is None or (klens.is_cuda and klens.dtype == torch.int32 and klens.is_contiguous() and klens.numel() * max(group, 1) >= R)
    if workspace is None:
        workspace = dec_attention_step_workspace(R, nh, n_split, q.device)
    ctx = torch.empty((R, nh * head_dim), dtype=torch.bfloat16, device=q.device) if ctx is None else ctx
    check(lib.ssak_dec_attention_step_grouped(ptr(q), q.stride(0), ptr(k), k.stride(1), k.stride(0), ptr(v), v.stride(1), v.stride(0), int(n_keys),
                                              ptr(klens), R, int(nh), int(head_dim), int(n_split), group, ptr(workspace), workspace.numel() * 4,
                                              ptr(ctx), stream()))
    return ctx


def dec_beam_topk(logits, V: int, nb: int, *, done, cand_token, cand_logprob, eos_id: int, t: int = 0, suppress=None, begin_suppress=None,
                  first: bool = False, timestamps: bool = False, ts_begin: int = 0, no_timestamps_id: int = 0, max_initial: int = -1, tokens=None,
                  ts_last=None):
    """``ssak_dec_beam_topk`` on logits [B * nb, ldv] fp32: per row the ``K = nb + 1`` largest log-probs of the processed row into
    ``cand_token`` int32 / ``cand_logprob`` fp32 [B * nb, K], highest first, a tie to the lowest column, -1 / -inf in unused slots.
    ``timestamps``: the rules of :func:`dec_timestamp_step` on ``tokens[:, :t]`` and ``ts_last`` [B * nb]; otherwise
    :func:`dec_greedy_step`'s.  ``done``: uint8 [B]; a done audio's rows are skipped."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    R, nb = logits.shape[0], int(nb)
    B = R // max(nb, 1)
    assert nb < 1 or B * nb == R
    assert done.dtype == torch.uint8 and done.numel() == B and done.is_contiguous()
    assert cand_token.dtype == torch.int32 and cand_logprob.dtype == torch.float32 and cand_token.shape == cand_logprob.shape
    assert cand_token.dim() == 2 and cand_token.shape[0] == R and cand_token.is_contiguous() and cand_logprob.is_contiguous()
    _assert_masks(V, suppress, begin_suppress)
    ldt = 0
    if tokens is not None:
        assert tokens.dtype == torch.int32 and tokens.is_contiguous() and tokens.shape[0] == R
        ldt = tokens.shape[1]
    assert ts_last is None or (ts_last.dtype == torch.int32 and ts_last.numel() == R and ts_last.is_contiguous())
    check(lib.ssak_dec_beam_topk(ptr(logits), logits.stride(0), B, nb, int(V), ptr(suppress), ptr(begin_suppress), int(bool(first)),
                                 int(bool(timestamps)), int(ts_begin), int(no_timestamps_id), int(max_initial), int(eos_id), ptr(tokens), ldt, int(t),
                                 ptr(ts_last), ptr(done), cand_token.shape[1], ptr(cand_token), ptr(cand_logprob), stream()))


def dec_beam_select(cand_token, cand_logprob, nb: int, V: int, *, sum_logprob, src, tokens, logprobs, t: int, fin_tokens, fin_logprobs, fin_len,
                    fin_sum, n_fin, done, n_unfinished, eos_id: int, pad_id: int, ts_last=None, ts_begin: int = 0, embed_tokens=None,
                    embed_positions=None, next_pos: int = 0, h_next=None):
    """``ssak_dec_beam_select``: one step of the beam search per audio on the candidates of :func:`dec_beam_topk` (the header states
    the rules).  Read and written on the device: ``sum_logprob`` fp32 [B, nb], ``tokens`` int32 / ``logprobs`` fp32 [B * nb, ldt]
    (permuted in place, column ``t`` written), ``ts_last`` int32 [B * nb] or None, the finished store ``fin_tokens`` / ``fin_logprobs``
    [B, nb, ldt], ``fin_len`` int32 / ``fin_sum`` fp32 [B, nb], ``n_fin`` int32 [B], ``done`` uint8 [B]; written: ``src`` int32 [B * nb],
    ``n_unfinished`` int32 [1], ``h_next`` [B * nb, D] bf16 (or None)."""
    R, nb = cand_token.shape[0], int(nb)
    B = R // max(nb, 1)
    assert nb < 1 or B * nb == R
    assert cand_token.dtype == torch.int32 and cand_logprob.dtype == torch.float32 and cand_token.shape == cand_logprob.shape
    assert cand_token.is_contiguous() and cand_logprob.is_contiguous()
    assert tokens.dtype == torch.int32 and logprobs.dtype == torch.float32 and tokens.shape == logprobs.shape and tokens.shape[0] == R
    assert tokens.is_contiguous() and logprobs.is_contiguous()
    ldt = tokens.shape[1]
    assert sum_logprob.dtype == torch.float32 and sum_logprob.numel() == R and sum_logprob.is_contiguous()
    assert src.dtype == torch.int32 and src.numel() == R and src.is_contiguous()
    assert fin_tokens.dtype == torch.int32 and fin_logprobs.dtype == torch.float32 and fin_tokens.numel() == R * ldt == fin_logprobs.numel()
    assert fin_tokens.is_contiguous() and fin_logprobs.is_contiguous()
    assert fin_len.dtype == torch.int32 and fin_len.numel() == R and fin_sum.dtype == torch.float32 and fin_sum.numel() == R
    assert n_fin.dtype == torch.int32 and n_fin.numel() == B and done.dtype == torch.uint8 and done.numel() == B
    assert n_unfinished.dtype == torch.int32
    assert ts_last is None or (ts_last.dtype == torch.int32 and ts_last.numel() == R and ts_last.is_contiguous())
    D, max_pos = _h_next_dims(embed_tokens, embed_positions, h_next, R)
    check(lib.ssak_dec_beam_select(ptr(cand_token), ptr(cand_logprob), B, nb, cand_token.shape[1], int(V), ptr(sum_logprob), ptr(src), ptr(tokens),
                                   ptr(logprobs), ldt, int(t), ptr(ts_last), int(ts_begin), ptr(fin_tokens), ptr(fin_logprobs), ptr(fin_len),
                                   ptr(fin_sum), ptr(n_fin), ptr(done), ptr(n_unfinished), ptr(embed_tokens), ptr(embed_positions), D, max_pos,
                                   int(next_pos), int(eos_id), int(pad_id), ptr(h_next), stream()))


def dec_kv_reorder(cache, src, nb: int, row_lo: int, row_hi: int):
    """``ssak_dec_kv_reorder``: the self-attention cache [layers, B * nb, cap, width] bf16 (any nested strides, the last 1) gathered by
    ``src`` int32 [B * nb] (global row indices) over the keys ``[row_lo, row_hi)``, in place."""
    assert cache.is_cuda and cache.dtype == torch.bfloat16 and cache.dim() == 4 and cache.stride(3) == 1
    assert src.dtype == torch.int32 and src.is_contiguous() and src.numel() == cache.shape[1]
    nb = int(nb)
    B = cache.shape[1] // max(nb, 1)
    assert nb < 1 or B * nb == cache.shape[1]
    check(lib.ssak_dec_kv_reorder(ptr(cache), ptr(src), cache.shape[0], B, nb, cache.shape[2], cache.shape[3], cache.stride(0), cache.stride(1),
                                  cache.stride(2), int(row_lo), int(row_hi), stream()))


def layernorm_fwd(y, res, gamma, beta, r_out=None, out=None, eps: float = 1e-5):
    """``ssak_layernorm_fwd``: r = res + y (either may be None) -> ``r_out``; ``out`` = LayerNorm(r) gamma + beta; [M, C] bf16 or fp32."""
    x = y if y is not None else res
    M, Cc = x.shape
    check(lib.ssak_layernorm_fwd(ptr(y), ptr(res), ptr(gamma), ptr(beta), ptr(r_out), ptr(out), M, Cc, float(eps), _row_dtype(x), stream()))
    return out if out is not None else r_out


# ------------------------------------------------------------------ Whisper training (ABI 650): the decoder's backward kernels
def dec_attention_fwd_lse(q, k, v, B: int, Lq: int, Lk: int, nh: int, *, klens=None, causal: bool = False, q_offset: int = 0,
                          head_dim: int = DEC_HEAD_DIM, ctx=None, lse=None):
    """``ssak_dec_attention_fwd_lse``: :func:`dec_attention_fwd` that also writes lse [B, nh, Lq] fp32, the natural-log
    log-sum-exp of each query's scaled, masked scores (what :func:`dec_attention_bwd` recomputes P from) -> (ctx, lse)."""
    lse = torch.empty((B, nh, Lq), dtype=torch.float32, device=q.device) if lse is None else lse
    return _dec_attention_fwd(q, k, v, B, Lq, Lk, nh, klens, causal, q_offset, head_dim, ctx, lse)


def dec_attention_bwd(q, k, v, ctx, lse, dctx, dq, dk, dv, B: int, Lq: int, Lk: int, nh: int, *, klens=None, causal: bool = False,
                      q_offset: int = 0, head_dim: int = DEC_HEAD_DIM, delta=None):
    """``ssak_dec_attention_bwd``: q, k, v and the mask as the forward took them, ctx / lse as it wrote them, dctx [B * Lq, nh * 64]
    -> dq [B * Lq, .], dk / dv [B * Lk, .] bf16 written into the caller's 2-D tensors or column slices (their row strides are
    passed on; rows of dk / dv at keys >= klens[b] are written as zeros).  Returns delta [B, nh, Lq] fp32."""
    for t in (q, k, v, dq, dk, dv):
        assert t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 2 and t.stride(1) == 1
    for t in (ctx, dctx):
        assert t.dtype == torch.bfloat16 and t.is_contiguous() and t.shape == (B * Lq, nh * head_dim)
    assert q.shape[0] == B * Lq and k.shape[0] == B * Lk and v.shape[0] == B * Lk, "q holds B * Lq rows, k and v B * Lk"
    assert dq.shape[0] == B * Lq and dk.shape[0] == B * Lk and dv.shape[0] == B * Lk
    assert lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() == B * nh * Lq
    kl_h = None if klens is None else _host_i32(klens, B, "klens")
    kl_d = None if kl_h is None else torch.from_numpy(kl_h).to(q.device)
    delta = torch.empty((B, nh, Lq), dtype=torch.float32, device=q.device) if delta is None else delta
    assert delta.dtype == torch.float32 and delta.is_contiguous() and delta.numel() == B * nh * Lq
    check(lib.ssak_dec_attention_bwd(ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), int(Lk), ptr(kl_d), _hp(kl_h), B, int(Lq),
                                     int(nh), int(head_dim), int(bool(causal)), int(q_offset), ptr(ctx), ptr(lse), ptr(dctx), ptr(dq),
                                     dq.stride(0), ptr(dk), dk.stride(0), ptr(dv), dv.stride(0), ptr(delta), stream()))
    return delta


def dec_ce_bwd(logits: torch.Tensor, V: int, targets, grad_scale: float = 1.0, dlogits=None, loss_sum=None, want_loss: bool = True):
    """``ssak_dec_ce_bwd`` on fp32 logits [R, ldv] (the first V columns valid) with host ``targets`` [R] (negative: ignored) ->
    (dlogits [R, ldd] bf16, row_loss [R] fp32 = -logprob, loss_sum [1] fp32).  ``loss_sum`` is added to when given (zeros
    otherwise); ``dlogits`` defaults to ldd = ldv.  ``want_loss=False``: dlogits alone, one launch -> (dlogits, None, None)."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    R, dev = logits.shape[0], logits.device
    tg_h = _host_i32(targets, R, "targets")
    tg_d = torch.from_numpy(tg_h).to(dev)
    dlogits = torch.empty((R, logits.shape[1]), dtype=torch.bfloat16, device=dev) if dlogits is None else dlogits
    assert dlogits.dtype == torch.bfloat16 and dlogits.dim() == 2 and dlogits.stride(1) == 1 and dlogits.shape[0] == R
    row_loss = torch.empty(R, dtype=torch.float32, device=dev) if want_loss else None
    loss_sum = None if not want_loss else torch.zeros(1, dtype=torch.float32, device=dev) if loss_sum is None else loss_sum
    check(lib.ssak_dec_ce_bwd(ptr(logits), R, int(V), logits.stride(0), ptr(tg_d), _hp(tg_h), float(grad_scale), ptr(dlogits),
                              dlogits.stride(0), ptr(row_loss), ptr(loss_sum), stream()))
    return dlogits, row_loss, loss_sum


def dec_embed_csr(ids):
    """ids [B, L] (or flat) -> (uniq, offsets, rows) int32: the distinct ids ascending, and for each the indices of the rows that
    hold it, ascending, as one CSR -- the fixed summation order of :func:`dec_embed_bwd`."""
    flat = np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)
    order = np.argsort(flat, kind="stable")  # stable: equal ids keep their rows ascending
    uniq, counts = np.unique(flat, return_counts=True)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    return uniq.astype(np.int32), offsets.astype(np.int32), order.astype(np.int32)


def dec_embed_bwd(dh: torch.Tensor, ids, d_embed_tokens: torch.Tensor, d_embed_positions: torch.Tensor, pos_offset: int = 0):
    """``ssak_dec_embed_bwd``: dh [B * L, D] bf16 and the host ``ids`` [B, L] of the forward -> d_embed_tokens [Vp, D] fp32 += the
    rows of each token (fixed order: :func:`dec_embed_csr`), d_embed_positions [max_pos, D] fp32 += the sums over the batch."""
    ids_np = ids.detach().cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)
    B, L = ids_np.shape
    D = dh.shape[1]
    assert dh.is_cuda and dh.dtype == torch.bfloat16 and dh.is_contiguous() and dh.shape[0] == B * L
    for t in (d_embed_tokens, d_embed_positions):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[1] == D
    host = [np.ascontiguousarray(a) for a in dec_embed_csr(ids_np)]
    dev = [torch.from_numpy(a).to(dh.device) for a in host]
    check(lib.ssak_dec_embed_bwd(ptr(dh), B, L, D, d_embed_tokens.shape[0], d_embed_positions.shape[0], int(pos_offset), ptr(dev[0]),
                                 ptr(dev[1]), ptr(dev[2]), _hp(host[0]), _hp(host[1]), _hp(host[2]), host[0].shape[0], ptr(d_embed_tokens),
                                 ptr(d_embed_positions), stream()))


def layernorm_fwd_stats(y, res, gamma, beta, out, mean, rstd, r_out=None, eps: float = 1e-5):
    """``ssak_layernorm_fwd_stats``: :func:`layernorm_fwd` that saves mean / rstd [M] fp32 for :func:`layernorm_bwd`."""
    x = y if y is not None else res
    M, Cc = x.shape
    check(lib.ssak_layernorm_fwd_stats(ptr(y), ptr(res), ptr(gamma), ptr(beta), ptr(r_out), ptr(out), ptr(mean), ptr(rstd), M, Cc, float(eps),
                                       _row_dtype(x), stream()))
    return out


def layernorm_bwd(g1, g2, r, mean, rstd, gamma, g_res, dr, dgamma, dbeta, workspace=None):
    """``ssak_layernorm_bwd``: dr = LN_bwd(g1 + g2) + g_res (g2, g_res may be None); dgamma / dbeta [C] fp32 += the column sums."""
    M, Cc = r.shape
    ws = workspace if workspace is not None else _ws(lib.ssak_layernorm_bwd_workspace_bytes(Cc), r.device)
    check(lib.ssak_layernorm_bwd(ptr(g1), ptr(g2), ptr(r), ptr(mean), ptr(rstd), ptr(gamma), ptr(g_res), ptr(dr), ptr(dgamma), ptr(dbeta), M, Cc,
                                 _row_dtype(r), ptr(ws), ws.numel(), stream()))
    return dr


# ------------------------------------------------------------------ Whisper LoRA: the adapter around a frozen nn.Linear
LORA_SITE_BASE = 4096  # dropout sites of the decoder's adapters: LORA_SITE_BASE + 4 * layer + which (the encoder engine's own
#                        sites are 1 .. 3 and 16 + 4 * layer + 0 .. 3, the classification head's 4 and 5)


def _lora_dims(A: torch.Tensor, B: torch.Tensor, dtype):
    assert A.is_cuda and B.is_cuda and A.dtype == dtype and B.dtype == dtype and A.is_contiguous() and B.is_contiguous()
    assert A.dim() == 2 and B.dim() == 2 and A.shape[0] == B.shape[1], "A [r, D_in] and B [D_out, r]"
    return A.shape[0], A.shape[1], B.shape[0]


def _rows_bf16(t: torch.Tensor, M: int, width: int, what: str):
    assert t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 2 and t.stride(1) == 1 and t.shape == (M, width), \
        f"{what}: [{M}, {width}] bf16 (a column slice is fine), got {tuple(t.shape)} {t.dtype}"


def lora_fwd(x, A, B, y, scaling: float, t=None, seed: int = 0, site: int = 0, drop_p: float = 0.0):
    """``ssak_lora_fwd``: y [M, D_out] (a 2-D tensor or a column slice, updated in place) += scaling * bf16(dropout(x) A^T) B^T;
    ``t`` [M, r] bf16 contiguous receives the rounded down-projection (None: not kept) -> y."""
    r, D_in, D_out = _lora_dims(A, B, torch.bfloat16)
    M = x.shape[0]
    _rows_bf16(x, M, D_in, "x")
    _rows_bf16(y, M, D_out, "y")
    assert t is None or (t.dtype == torch.bfloat16 and t.is_contiguous() and t.shape == (M, r))
    check(lib.ssak_lora_fwd(ptr(x), x.stride(0), ptr(A), ptr(B), ptr(y), y.stride(0), ptr(t), M, D_in, D_out, r, float(scaling),
                            C.c_uint64(int(seed)), int(site), float(drop_p), stream()))
    return y


def lora_bwd_input(dy, A, B, dt, scaling: float, dx=None, accumulate: bool = False, seed: int = 0, site: int = 0, drop_p: float = 0.0):
    """``ssak_lora_bwd_input``: dt [M, r] bf16 = scaling * dy B; with ``dx`` [M, D_in] (a tensor or a column slice):
    dx (+)= keep * (dt A) / (1 - p) -> dt."""
    r, D_in, D_out = _lora_dims(A, B, torch.bfloat16)
    M = dy.shape[0]
    _rows_bf16(dy, M, D_out, "dy")
    assert dt.dtype == torch.bfloat16 and dt.is_contiguous() and dt.shape == (M, r)
    if dx is not None:
        _rows_bf16(dx, M, D_in, "dx")
    check(lib.ssak_lora_bwd_input(ptr(dy), dy.stride(0), ptr(A), ptr(B), ptr(dt), ptr(dx), 0 if dx is None else dx.stride(0), int(bool(accumulate)),
                                  M, D_in, D_out, r, float(scaling), C.c_uint64(int(seed)), int(site), float(drop_p), stream()))
    return dt


def lora_bwd_weights(dy, t, dt, x, dA, dB, scaling: float, seed: int = 0, site: int = 0, drop_p: float = 0.0, workspace=None):
    """``ssak_lora_bwd_weights``: dB [D_out, r] fp32 = scaling * dy^T t, dA [r, D_in] fp32 = dt^T dropout(x) (both written; the mask
    is regenerated from ``seed`` / ``site``)."""
    assert dA.is_cuda and dB.is_cuda and dA.dtype == torch.float32 and dB.dtype == torch.float32 and dA.is_contiguous() and dB.is_contiguous()
    assert dA.dim() == 2 and dB.dim() == 2 and dA.shape[0] == dB.shape[1], "dA [r, D_in] and dB [D_out, r]"
    r, D_in, D_out = dA.shape[0], dA.shape[1], dB.shape[0]
    M = x.shape[0]
    _rows_bf16(x, M, D_in, "x")
    _rows_bf16(dy, M, D_out, "dy")
    for a in (t, dt):
        assert a.dtype == torch.bfloat16 and a.is_contiguous() and a.shape == (M, r)
    ws = workspace if workspace is not None else _ws(lib.ssak_lora_bwd_weights_workspace_bytes(M, D_in, D_out, r), x.device)
    check(lib.ssak_lora_bwd_weights(ptr(dy), dy.stride(0), ptr(t), ptr(dt), ptr(x), x.stride(0), ptr(dB), ptr(dA), M, D_in, D_out, r,
                                    float(scaling), C.c_uint64(int(seed)), int(site), float(drop_p), ptr(ws), ws.numel(), stream()))


def lora_merge(w_master, A, B, w_out, scaling: float, w_out_f32=None):
    """``ssak_lora_merge``: w_out [D_out, D_in] bf16 = bf16(w_master + scaling * B A) from the fp32 masters; ``w_out_f32`` (None, or
    ``w_master`` itself) receives the value before the rounding -> w_out."""
    r, D_in, D_out = _lora_dims(A, B, torch.float32)
    assert w_master.is_cuda and w_master.dtype == torch.float32 and w_master.is_contiguous() and w_master.shape == (D_out, D_in)
    assert w_out.is_cuda and w_out.dtype == torch.bfloat16 and w_out.is_contiguous() and w_out.shape == (D_out, D_in)
    assert w_out_f32 is None or (w_out_f32.dtype == torch.float32 and w_out_f32.is_contiguous() and w_out_f32.shape == (D_out, D_in))
    check(lib.ssak_lora_merge(ptr(w_master), ptr(A), ptr(B), ptr(w_out), ptr(w_out_f32), D_in, D_out, r, float(scaling), stream()))
    return w_out


# ------------------------------------------------------------------ test-only: the dropout bits of one site
def debug_dropout_mask(seed: int, site: int, p: float, rows: int, cols: int, device):
    """(keep [rows, cols] uint8, scale) of one dropout site (``ssak_debug_dropout_mask``)."""
    keep = torch.empty((rows, cols), dtype=torch.uint8, device=device)
    scale = C.c_float()
    check(lib.ssak_debug_dropout_mask(C.c_uint64(int(seed)), int(site), float(p), rows, cols, ptr(keep), C.byref(scale), stream()))
    return keep, scale.value


# ------------------------------------------------------------------ test-only: the row kernels of norm_act.hip (ABI 540)
def _row_dtype(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return 0
    if t.dtype == torch.float32:
        return 1
    raise TypeError(f"row kernels take bf16 or fp32 activations, not {t.dtype}")


def debug_layernorm_fwd(y, res, gamma, beta, r_out=None, out=None, mean=None, rstd=None, *, eps=1e-5, seed=0, pre=(0, 0.0),
                        mid=(0, 0.0), post=(0, 0.0), post_gelu=False):
    """One ``k_layernorm_fwd_t`` launch into the caller's buffers (``ssak_debug_layernorm_fwd``).  Sites are (site id, p)."""
    x = y if y is not None else res
    M, C = x.shape
    check(lib.ssak_debug_layernorm_fwd(ptr(y), ptr(res), ptr(gamma), ptr(beta), ptr(r_out), ptr(out), ptr(mean), ptr(rstd), M, C,
                                       float(eps), seed, pre[0], float(pre[1]), mid[0], float(mid[1]),
                                       post[0], float(post[1]), int(bool(post_gelu)), _row_dtype(x), stream()))


def debug_layernorm_bwd(g1, g2, r, mean, rstd, gamma, g_res, dr, dy, dgamma, dbeta, dy_colsum=None, post_gelu_beta=None, *, seed=0,
                        pre=(0, 0.0), mid=(0, 0.0), post=(0, 0.0), queued=False, workspace=None):
    """One ``k_layernorm_bwd_t`` launch (+ its column-sum second stage, queued or direct) into the caller's buffers."""
    M, Cc = r.shape
    nbytes = lib.ssak_debug_layernorm_bwd_workspace_bytes(Cc)
    ws = workspace if workspace is not None else _ws(nbytes, r.device)
    check(lib.ssak_debug_layernorm_bwd(ptr(g1), ptr(g2), ptr(r), ptr(mean), ptr(rstd), ptr(gamma), ptr(g_res), ptr(dr), ptr(dy),
                                       ptr(dgamma), ptr(dbeta), ptr(dy_colsum), ptr(post_gelu_beta), M, Cc, seed, pre[0], float(pre[1]),
                                       mid[0], float(mid[1]), post[0], float(post[1]), int(bool(queued)), _row_dtype(r), ptr(ws),
                                       ws.numel(), stream()))


def debug_softmax_fwd(S, P, Pd, klens, cols: int, rows_per_batch: int = 1, *, seed=0, site=0, p=0.0):
    """``k_softmax_fwd_t`` on S [rows, ld] (ld = row stride) into P (and Pd)."""
    rows, ld = S.shape
    check(lib.ssak_debug_softmax_fwd(ptr(S), ptr(P), ptr(Pd), ptr(klens), rows, cols, ld, rows_per_batch, seed, site, float(p),
                                     _row_dtype(S), stream()))


def debug_softmax_bwd(dPd, P, dS, cols: int, *, seed=0, site=0, p=0.0):
    rows, ld = P.shape
    check(lib.ssak_debug_softmax_bwd(ptr(dPd), ptr(P), ptr(dS), rows, cols, ld, seed, site, float(p), _row_dtype(P), stream()))


def debug_gelu(x: torch.Tensor, dtype: torch.dtype):
    """gelu(x), gelu'(x) [fp32] as the kernels of storage type ``dtype`` evaluate them."""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    y, d = torch.empty_like(x), torch.empty_like(x)
    check(lib.ssak_debug_gelu(ptr(x), x.numel(), ptr(y), ptr(d), 0 if dtype == torch.bfloat16 else 1, stream()))
    return y, d


# ------------------------------------------------------------------ test-only: the adapter layer's closing row kernel (ABI 590)
def test_attn_adapter_fwd(y, res, ln_g, ln_b, w1, b1, w2, b2, next_g, next_b, r_out, out, mean=None, rstd=None, *, eps_adapter=1e-5,
                          eps_next=1e-5):
    """One ``k_attn_adapter_fwd_t`` launch into the caller's buffers (``ssak_test_attn_adapter_fwd``): y (or None), res, r_out, out
    [M, H] and w1 [A, H], w2 [H, A] all bf16 or all fp32; the LayerNorm affines and the biases fp32."""
    M, H = res.shape
    A = w1.shape[0]
    dt = _row_dtype(res)
    assert all(t is None or t.dtype == res.dtype for t in (y, w1, w2, r_out, out)), "activations and W1 / W2 share one storage type"
    check(lib.ssak_test_attn_adapter_fwd(ptr(y), ptr(res), ptr(ln_g), ptr(ln_b), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(next_g),
                                         ptr(next_b), ptr(r_out), ptr(out), ptr(mean), ptr(rstd), M, H, A, float(eps_adapter),
                                         float(eps_next), dt, stream()))


test_attn_adapter_fwd.__test__ = False  # (a binding, not a test: keep collectors that import this module away from it)


# ------------------------------------------------------------------ test-only: the grouped positional convolution (ABI 550)
def debug_posconv_prepare(g: torch.Tensor, v: torch.Tensor, G: int, dtype: torch.dtype = torch.bfloat16):
    """``k_posconv_prepare_t``: g [K], v [H, cg, K] fp32 -> (wf [H, K, cg], wb [G, cg, K, cg], norms); norms[:K] = ||v_k||^2, the
    rest is the scratch ``debug_posconv_weight_bwd`` needs.  Outputs start from NaN."""
    H, cg, K = v.shape
    nan = float("nan")
    wf = torch.full((H, K, cg), nan, dtype=dtype, device=v.device)
    wb = torch.full((G, cg, K, cg), nan, dtype=dtype, device=v.device)
    norms = torch.full(((2 + H) * K,), nan, dtype=torch.float32, device=v.device)
    check(lib.ssak_debug_posconv_prepare(ptr(g), ptr(v), ptr(wf), ptr(wb), ptr(norms), H, G, K, _row_dtype(wf), stream()))
    return wf, wb, norms


def debug_posconv_pack(h: torch.Tensor, B: int, F: int, G: int, K: int):
    """``k_posconv_pack_t`` on h [B * F, H] (bf16 or fp32) -> the packed [G, K / 2 + B (F + K) + K, cg], written over NaN."""
    H = h.shape[1]
    pg = torch.full((G, K // 2 + B * (F + K) + K, H // G), float("nan"), dtype=h.dtype, device=h.device)
    check(lib.ssak_debug_posconv_pack(ptr(h), ptr(pg), B, F, H, G, K, _row_dtype(h), stream()))
    return pg


def debug_posconv_workspace(B: int, F: int, H: int, G: int, K: int, device):
    """A workspace for ``debug_posconv_direct`` / ``debug_posconv_wgrad``, every byte 0xFF (NaN as bf16 and as fp32)."""
    nbytes = lib.ssak_debug_posconv_workspace_bytes(B, F, H, G, K)
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=device)


def debug_posconv_direct(h, w, bias, out, pre, B: int, F: int, G: int, K: int, *, row0=0, gelu=False, workspace=None):
    """pack + fragment order + one ``k_posconv_direct`` launch into the caller's out / pre ([B * F, H] bf16; pre may be None).
    w: bf16 in the wf layout [H, K, cg] (forward) or the wb layout [G, cg, K, cg] (input gradient, row0 = 1)."""
    H = h.shape[1]
    ws = workspace if workspace is not None else debug_posconv_workspace(B, F, H, G, K, h.device)
    check(lib.ssak_debug_posconv_direct(ptr(h), ptr(w), ptr(bias), ptr(out), ptr(pre), B, F, H, G, K, int(row0), int(bool(gelu)),
                                        ptr(ws), ws.numel(), stream()))


def debug_posconv_wgrad(h, dpre, dwf, B: int, F: int, G: int, K: int, *, workspace=None):
    """pack of both + ``k_posconv_wgrad_direct`` into dwf [G, K * cg, cg] fp32 (overwritten)."""
    H = h.shape[1]
    ws = workspace if workspace is not None else debug_posconv_workspace(B, F, H, G, K, h.device)
    check(lib.ssak_debug_posconv_wgrad(ptr(h), ptr(dpre), ptr(dwf), B, F, H, G, K, ptr(ws), ws.numel(), stream()))


def debug_posconv_weight_bwd(dwf, g, v, norms, dg, dv, G: int):
    """``k_posconv_weight_bwd``: dg [K], dv [H, cg, K] += the weight-norm backward of dwf; norms from ``debug_posconv_prepare``."""
    H, cg, K = v.shape
    check(lib.ssak_debug_posconv_weight_bwd(ptr(dwf), ptr(g), ptr(v), ptr(norms), ptr(dg), ptr(dv), H, G, K, stream()))


# ------------------------------------------------------------------ test-only: the trained feature encoder's kernels and the
# Whisper front end's data movers (ABI 570).  Every wrapper launches into the caller's buffers.
def debug_conv0_bwd_workspace(B: int, T: int, C_: int, device):
    """The scratch of ``debug_conv0_bwd``, every byte 0xFF (NaN as fp32 and as fp64)."""
    nbytes = lib.ssak_debug_conv0_bwd_workspace_bytes(B, T, C_)
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=device)


def debug_conv0_bwd(x, w, gamma, beta, dy, sums, dw, dgamma, dbeta, *, workspace=None):
    """``k_conv0_gn_gelu_bwd_t``: x [B, T], w [C, 10], dy [B, T0, C] (bf16 or fp32), sums [B, C, 2] float64 (mean, rstd);
    dw [C, 10], dgamma [C], dbeta [C] +=."""
    B, T = x.shape
    Cc = w.shape[0]
    ws = workspace if workspace is not None else debug_conv0_bwd_workspace(B, T, Cc, x.device)
    check(lib.ssak_debug_conv0_bwd(ptr(x), ptr(w), ptr(gamma), ptr(beta), ptr(dy), ptr(sums), ptr(dw), ptr(dgamma), ptr(dbeta), B, T, Cc,
                                   _row_dtype(dy), ptr(ws), ws.numel(), stream()))


def debug_conv0_wgrad(d, x, dw, stride: int, *, workspace=None):
    """``k_conv0_wgrad_t``: d [B, T0, C], x [B, T]; dw [C, ksize] +=."""
    B, T = x.shape
    Cc, ksize = dw.shape
    nbytes = lib.ssak_debug_conv0_wgrad_workspace_bytes(B, Cc, ksize)
    ws = workspace if workspace is not None else torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=x.device)
    check(lib.ssak_debug_conv0_wgrad(ptr(d), ptr(x), ptr(dw), B, T, Cc, ksize, int(stride), _row_dtype(d), ptr(ws), ws.numel(), stream()))


def debug_conv0_bias(x, w, bias, out):
    """``k_conv0_bias_t``: out [>= B * T0, C] = conv0(x) + bias (bias may be None)."""
    B, T = x.shape
    check(lib.ssak_debug_conv0_bias(ptr(x), ptr(w), ptr(bias), ptr(out), B, T, w.shape[0], _row_dtype(out), stream()))


def debug_col2im(dxcol, dx, k: int, s: int):
    """``k_col2im_t``: dxcol [B, Tout, k, C] -> dx [B, Tin, C]."""
    B, Tout, kk, Cc = dxcol.shape
    assert kk == k and dx.shape[0] == B and dx.shape[2] == Cc
    check(lib.ssak_debug_col2im(ptr(dxcol), ptr(dx), B, dx.shape[1], Tout, Cc, k, s, _row_dtype(dx), stream()))


def debug_sum_slabs(slabs, out):
    """``k_sum_slabs``: slabs [nb, n] fp32 -> out [n]."""
    nb, n = slabs.shape
    check(lib.ssak_debug_sum_slabs(ptr(slabs), nb, n, ptr(out), stream()))


def debug_conv_weight_rearrange(w, out):
    """``k_conv_weight_rearrange_t``: w [Co, Ci, k] fp32 -> out [Co, k, Ci] (bf16 or fp32)."""
    Co, Ci, k = w.shape
    check(lib.ssak_debug_conv_weight_rearrange(ptr(w), ptr(out), Co, Ci, k, _row_dtype(out), stream()))


def debug_conv_wgrad_unrearrange(dwr, g):
    """``k_conv_wgrad_unrearrange``: g [Co, Ci, k] += dwr [Co, k, Ci]."""
    Co, Ci, k = g.shape
    check(lib.ssak_debug_conv_wgrad_unrearrange(ptr(dwr), ptr(g), Co, Ci, k, stream()))


def debug_col2im_k3s2(dxcol, pre, out, Tin: int):
    """``k_col2im_k3s2_t``: dxcol [B, F, 3, H], pre [B * RS1, H] (one-row lead) -> out [B, RS1, H]."""
    B, F, _, H = dxcol.shape
    check(lib.ssak_debug_col2im_k3s2(ptr(dxcol), ptr(pre), ptr(out), B, F, Tin, out.shape[1], H, _row_dtype(out), stream()))


def debug_mel_to_cl(mel, cl, RS: int, lead: int):
    """``k_mel_to_cl_t``: mel [B, C, T] fp32 -> rows b RS + lead + t of cl [rows, C]."""
    B, Cc, T = mel.shape
    check(lib.ssak_debug_mel_to_cl(ptr(mel), ptr(cl), B, Cc, T, RS, lead, _row_dtype(cl), stream()))


def debug_add_rowvec(x, pos, out):
    """``k_add_rowvec_t``: out [B, F, H] = x + pos [F, H]."""
    B, F, H = x.shape
    check(lib.ssak_debug_add_rowvec(ptr(x), ptr(pos), ptr(out), B, F, H, _row_dtype(x), stream()))


def debug_copy_rows_padded(src, dst):
    """``k_copy_rows_padded_t``: src [B, F, H] -> dst [B, RS, H], rows >= F zero."""
    B, F, H = src.shape
    check(lib.ssak_debug_copy_rows_padded(ptr(src), ptr(dst), B, F, dst.shape[1], H, _row_dtype(src), stream()))


# ------------------------------------------------------------------ test-only: the engine's helper kernels (ABI 660).  Every
# wrapper launches into the caller's buffers; ``scratch`` is an fp32 tensor (or None: the atomic path of the column sum).
def debug_specaug_fwd(h, mask, flens, embed):
    """``k_specaug_fwd_t`` in place on h [B, F, C] (bf16 or fp32): mask [B, F] uint8 or None, flens [B] int32 or None, embed [C] fp32."""
    B, F, Cc = h.shape
    check(lib.ssak_debug_specaug_fwd(ptr(h), ptr(mask), ptr(flens), ptr(embed), B, F, Cc, _row_dtype(h), stream()))


def debug_specaug_bwd(dh, mask, flens, dembed, scratch=None, scratch_floats=None):
    """``k_specaug_bwd_t`` in place on dh [B, F, C]; dembed [C] fp32 +=.  ``scratch_floats`` defaults to the scratch's size."""
    B, F, Cc = dh.shape
    nf = (0 if scratch is None else scratch.numel()) if scratch_floats is None else int(scratch_floats)
    check(lib.ssak_debug_specaug_bwd(ptr(dh), ptr(mask), ptr(flens), ptr(dembed), B, F, Cc, _row_dtype(dh), ptr(scratch), nf, stream()))


def debug_colsum(X, N: int, out, scratch=None, scratch_floats=None, rowmask=None, flens=None, F: int = 0):
    """``k_colsum_t``: out [N] fp32 += the column sums of the first N columns of X [M, ld] (ld = X's row stride)."""
    M, ld = X.shape
    nf = (0 if scratch is None else scratch.numel()) if scratch_floats is None else int(scratch_floats)
    check(lib.ssak_debug_colsum(ptr(X), ld, M, N, ptr(out), ptr(scratch), nf, ptr(rowmask), ptr(flens), int(F), _row_dtype(X), stream()))


def debug_gelu_grad_mul(dy, pre, out, n: int):
    """``k_gelu_grad_mul_t``: out[:n] = dy[:n] * gelu'(pre[:n]) (flat tensors of one storage type)."""
    check(lib.ssak_debug_gelu_grad_mul(ptr(dy), ptr(pre), ptr(out), int(n), _row_dtype(dy), stream()))


def debug_add(a, b, out, n: int):
    """``k_add_t``: out[:n] = a[:n] + b[:n]."""
    check(lib.ssak_debug_add(ptr(a), ptr(b), ptr(out), int(n), _row_dtype(a), stream()))


def debug_transpose_batched(src_ptrs, dst_ptrs, R, Cs):
    """``k_transpose_bf16_batched``: dst[i] [C, R] = src[i] [R, C]^T; device addresses (``data_ptr()``, any alignment) and shapes."""
    n = len(src_ptrs)
    assert len(dst_ptrs) == n and len(R) == n and len(Cs) == n
    check(lib.ssak_debug_transpose_batched(n, (C.c_void_p * n)(*src_ptrs), (C.c_void_p * n)(*dst_ptrs), (C.c_int * n)(*R),
                                           (C.c_int * n)(*Cs), stream()))


def debug_reduce(jobs, call_sizes, use_sink: bool):
    """``k_reduce`` on jobs = [(partial, out, stride, slots, ncols), ...] (fp32 tensors), issued as consecutive calls of
    ``call_sizes`` jobs, under a local ReduceSink that is flushed at the end (``use_sink``) or directly.  Returns (jobs queued,
    jobs run directly)."""
    n, nc = len(jobs), len(call_sizes)
    queued, direct = C.c_int(-1), C.c_int(-1)
    check(lib.ssak_debug_reduce(n, (C.c_void_p * n)(*[j[0].data_ptr() for j in jobs]), (C.c_void_p * n)(*[j[1].data_ptr() for j in jobs]),
                                (C.c_long * n)(*[int(j[2]) for j in jobs]), (C.c_int * n)(*[int(j[3]) for j in jobs]),
                                (C.c_int * n)(*[int(j[4]) for j in jobs]), nc, (C.c_int * nc)(*[int(v) for v in call_sizes]),
                                int(bool(use_sink)), C.byref(queued), C.byref(direct), stream()))
    return queued.value, direct.value
