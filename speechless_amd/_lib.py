"""ctypes binding of include/speechless_hip.h.  There is NO fallback: if the HIP library is missing or a call
fails, this raises -- the product path never computes on the CPU."""
import ctypes
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p
from pathlib import Path

# torch FIRST: its wheel bundles its own libamdhip64.so.7 / libhsa-runtime64.  libspeechless_hip.so needs the same
# SONAME, and a process must hold exactly ONE HIP runtime -- the one that owns the tensors' memory and streams.
# Loading ours first would pull /opt/rocm's runtime in and torch would then find "no ROCm-capable device".
import torch  # noqa: F401  (plumbing: device memory, streams, torch.distributed)

import os

from .launch_list import HipLibraryError, raise_status  # noqa: F401  (the error every failing library call raises)

# SL_LIB_PATH: experiments only (a probe build of the library next to the real one)
LIB_PATH = Path(os.environ.get("SL_LIB_PATH") or Path(__file__).resolve().parent / "libspeechless_hip.so")

SL_BF16 = 0
SL_F32 = 1
SL_F16 = 2

# sl_stft `mode` (include/speechless_hip.h)
STFT_POWER, STFT_AMPLITUDE, STFT_COMPLEX, STFT_POWER_LEVEL = 0, 1, 2, 3

EPI_NONE = 0
EPI_BIAS = 1
EPI_BIAS_RELU = 2
EPI_RELU_MASK = 3
EPI_BIAS_ELU = 4
EPI_ELU_MASK = 5

# sl_conv1d_nt's out_f32: the output in the element type, as fp32 rows, or as hi + lo planes out of the epilogue
NT_OUT_ELEM, NT_OUT_F32, NT_OUT_PLANES = 0, 1, 2
# sl_split3 / sl_splitf16 `mode`: fp32 rows into planes as they are, through ReLU / ELU, or times the ReLU / ELU derivative
# taken from the stored activation (`mask`)
SPLIT_COPY, SPLIT_RELU, SPLIT_ELU, SPLIT_RELU_MASK, SPLIT_ELU_MASK = 0, 1, 2, 3, 4
# sl_split3_dropout / sl_splitf16_dropout `mode`: forward; the 1 / (1 - rate) left behind a ReLU mask; keep * elu' behind an ELU
DROP_FORWARD, DROP_SCALE, DROP_ELU_BACKWARD = 0, 1, 2


class AdamLayer(ctypes.Structure):
    """Mirror of sl_adam_layer (include/speechless_hip.h)."""
    _fields_ = [("offset", c_int64), ("w_fwd", c_void_p), ("w_dgrad", c_void_p), ("k", c_int32), ("cin_pad", c_int32),
                ("cout_pad", c_int32)]


class OptRule(ctypes.Structure):
    """Mirror of sl_opt_rule (include/speechless_hip.h)."""
    _fields_ = [("rule", c_int32), ("lr", c_float), ("momentum", c_float), ("nesterov", c_int32), ("rho", c_float),
                ("beta1", c_float), ("beta2", c_float), ("eps", c_float)]


# SL_OPT_* (include/speechless_hip.h); the number of fp32 state slots per parameter of each rule
OPT_RULES = {"adam": 0, "sgd": 1, "rmsprop": 2, "adagrad": 3, "adadelta": 4, "adamax": 5}
OPT_SLOTS = {"adam": 2, "sgd": 1, "rmsprop": 1, "adagrad": 1, "adadelta": 2, "adamax": 2}


class BgwLayer(ctypes.Structure):
    """Mirror of sl_bgw_layer (include/speechless_hip.h)."""
    _fields_ = [("w_off", c_int64), ("b_off", c_int64), ("k", c_int32), ("cin_pad", c_int32), ("cout_pad", c_int32),
                ("tap", c_int32)]


class NormRange(ctypes.Structure):
    """Mirror of sl_norm_range (include/speechless_hip.h)."""
    _fields_ = [("offset", c_int64), ("count", c_int64)]


class ConvGeom(ctypes.Structure):
    """Mirror of sl_conv_geom (include/speechless_hip.h)."""
    _fields_ = [
        ("batch", c_int32),
        ("t_out", c_int32),
        ("taps", c_int32),
        ("cin", c_int32),
        ("cout", c_int32),
        ("x_row0", c_int32),
        ("x_row_stride", c_int32),
        ("x_batch_stride", c_int64),
        ("y_row0", c_int32),
        ("y_row_stride", c_int32),
        ("y_batch_stride", c_int64),
        ("acc_scale", c_float),
    ]

    def copy_from(self, src):
        for name, _ in ConvGeom._fields_:
            setattr(self, name, getattr(src, name))

    def copy(self):
        g = ConvGeom()
        g.copy_from(self)
        return g


class BeamLm(ctypes.Structure):
    """Mirror of sl_beam_lm (include/speechless_hip.h): device pointers of the flat scorer tables."""
    _fields_ = [("trie_child", c_void_p), ("trie_min", c_void_p), ("trie_word", c_void_p), ("ngrams", c_void_p),
                ("n_trie_nodes", c_int64), ("ngram_slots", c_int64), ("order", c_int), ("bos", c_int), ("eos", c_int),
                ("space_label", c_int), ("oov_score", c_float), ("lm_weight", c_float), ("word_count_weight", c_float),
                ("valid_word_count_weight", c_float)]


class WgradJob(ctypes.Structure):
    """Mirror of sl_wgrad_job (include/speechless_hip.h)."""
    _fields_ = [("x", c_void_p), ("g", c_void_p), ("dw", c_void_p), ("geom", ConvGeom)]


# name -> (restype, argtypes); every symbol include/speechless_hip.h declares
SIGNATURES = {
    "sl_version": (c_int, []),
    "sl_profile_next_kernel": (c_int, [c_void_p, c_void_p]),
    "sl_output_softmax_supported": (c_int, [POINTER(ConvGeom), c_int, c_int]),
    "sl_output_softmax_select": (c_int, [c_int]),
    "sl_output_softmax": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(ConvGeom), c_int,
                                  c_int, c_int64, c_float, c_int, c_void_p]),
    "sl_last_error": (c_char_p, []),
    "sl_conv1d_nt_workspace_bytes": (c_size_t, [POINTER(ConvGeom), c_int, c_int]),
    "sl_conv1d_nt": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(ConvGeom), c_int, c_int, c_int,
                             c_int, c_void_p, c_size_t, c_void_p]),
    "sl_conv1d_chain_supported": (c_int, [POINTER(ConvGeom), c_int, c_int]),
    "sl_conv1d_chain_select": (c_int, [c_int]),
    "sl_conv1d_chain_plan": (c_int, [POINTER(ConvGeom), c_int, c_int]),
    "sl_conv1d_chain": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                                POINTER(ConvGeom), c_int, c_int, c_int, c_void_p]),
    "sl_conv1d_wgrad_workspace_bytes": (c_size_t, [POINTER(ConvGeom), c_int, c_int]),
    "sl_conv1d_wgrad": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(ConvGeom), c_int, c_int, c_void_p, c_size_t,
                                c_void_p]),
    "sl_conv1d_wgrad_grouped_workspace_bytes": (c_size_t, [POINTER(ConvGeom), c_int, c_int]),
    "sl_conv1d_wgrad_grouped": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(ConvGeom), c_int, c_int64, c_int64,
                                        c_int64, c_int, c_void_p, c_size_t, c_void_p]),
    "sl_bias_grad_workspace_bytes": (c_size_t, [POINTER(ConvGeom)]),
    "sl_bias_grad": (c_int, [c_void_p, c_void_p, POINTER(ConvGeom), c_int, c_void_p, c_size_t, c_void_p]),
    "sl_pack_weights": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "sl_dropout": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_float, ctypes.c_uint64, c_void_p]),
    "sl_scale": (c_int, [c_void_p, c_size_t, c_int, c_float, c_void_p]),
    "sl_elu_dropout_backward": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_float, ctypes.c_uint64, c_void_p]),
    "sl_pack_input": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_int, c_void_p]),
    "sl_wave_frames": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, c_int, c_void_p]),
    "sl_pack_input_ones": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_int, c_int, c_void_p]),
    "sl_softmax_logq": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64, c_float,
                                c_void_p]),
    "sl_ctc_select": (c_int, [c_int]),
    "sl_ctc_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sl_ctc_loss_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                 c_int, c_int, c_int, c_int, c_int64, c_int, c_float, c_float, c_void_p, c_size_t,
                                 c_void_p]),
    "sl_greedy_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                 c_void_p]),
    "sl_ctc_align_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sl_ctc_align": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                             c_void_p, c_size_t, c_void_p]),
    "sl_ctc_align_long_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sl_ctc_align_long": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                  c_void_p, c_size_t, c_void_p]),
    "sl_ctc_segment_scores_workspace_bytes": (c_size_t, [c_int, c_int]),
    # logq, labels, input_len, segments, log_posterior, batch, t_out, k, l_max, n_segments, seg_l_max, workspace, bytes, stream
    "sl_ctc_segment_scores": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_void_p, c_size_t, c_void_p]),
    "sl_ctc_spot_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    # logq, input_len, queries, query_len, query_utt, min_score, hits, hit_score, n_hits, frame_score, frame_begin, batch, t_out,
    # k, n_queries, q_max, max_hits, workspace, bytes, stream
    "sl_ctc_spot": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "sl_asg_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    # probs, logq, trans, init, labels, label_len, input_len, loss, dlogits, dtrans, dinit; then sl_ctc_loss_grad's tail
    "sl_asg_loss_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, c_int, c_float, c_float,
                                 c_void_p, c_size_t, c_void_p]),
    "sl_asg_viterbi_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sl_asg_viterbi": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                               c_size_t, c_void_p]),
    "sl_asg_align_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    # logq, trans, init, labels, label_len, input_len, path, score
    "sl_asg_align": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                             c_int, c_void_p, c_size_t, c_void_p]),
    "sl_asg_align_long_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sl_asg_align_long": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                  c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "sl_asg_segment_scores_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    # logq, trans, init, labels, input_len, segments, log_posterior, batch, t_out, k, l_max, n_segments, seg_l_max, workspace,
    # bytes, stream
    "sl_asg_segment_scores": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                      c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "sl_edit_distance_supported": (c_int, [c_int, c_int]),
    "sl_edit_distance": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "sl_ctc_beam_search_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "sl_ctc_beam_search": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, POINTER(BeamLm),
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sl_asg_beam_search_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    # logq, trans, init, input_len, batch, t_out, k, beam_width, lm, out, out_len, score, workspace, bytes, stream
    "sl_asg_beam_search": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(BeamLm),
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sl_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_float, c_float, c_float,
                             c_float, c_void_p]),
    "sl_adam_pack_layer": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_int, c_int, c_float, c_float, c_float, c_float, c_void_p]),
    "sl_stft_power_db": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64,
                                 c_float, c_void_p]),
    # audio, offsets, lengths, out, batch, max_frames, n_fft, hop, row_stride, batch_stride, mode, min_db, stream
    "sl_stft": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_int, c_float,
                        c_void_p]),
    "sl_istft_tile_frames": (c_int, [c_int, c_int]),
    # spec, frames, audio, out_offsets, batch, max_frames, n_fft, hop, row_stride, batch_stride, stream
    "sl_istft": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_void_p]),
    "sl_z_normalize_workspace_bytes": (c_size_t, [c_int]),
    "sl_z_normalize": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64, c_void_p, c_size_t,
                               c_void_p]),
    # audio, in_offsets, in_lengths, out, out_offsets, bank, batch, p, q, left, width, stream
    "sl_resample_polyphase": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                      c_int, c_void_p]),
    "sl_bias_grad_from_wgrad": (c_int, [c_void_p, POINTER(BgwLayer), c_int, c_int, c_void_p]),
    "sl_adam_pack_layers": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(AdamLayer), c_int, c_int, c_int,
                                    c_float, c_float, c_float, c_float, c_void_p]),
    "sl_set_available_cus": (c_int, [c_int]),
    "sl_conv1d_backward_1x1_supported": (c_int, [POINTER(ConvGeom), c_int, c_int]),
    "sl_conv1d_backward_1x1_workspace_bytes": (c_size_t, [POINTER(ConvGeom), c_int, c_int, c_int]),
    "sl_conv1d_backward_1x1": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(ConvGeom), c_int, c_int,
                                       c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "sl_conv1d_backward_1x1_part": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(ConvGeom), c_int, c_int,
                                            c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "sl_split3": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_int64, c_int, c_void_p]),
    "sl_split3_pack_input": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_void_p]),
    "sl_split3_weights": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sl_split3_assemble": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "sl_split3_pack_weights": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "sl_split3_adam_pack_layers": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(AdamLayer), c_int, c_int, c_float,
                                           c_float, c_float, c_float, c_void_p]),
    "sl_split3_wgrad_combine": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p]),
    "sl_split3_bias_grad_workspace_bytes": (c_size_t, [c_int]),
    "sl_split3_dropout": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_float, ctypes.c_uint64, c_void_p]),
    "sl_split3_bias_grad": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64, c_void_p, c_size_t, c_void_p]),
    "sl_conv1d_wgrad_multi_workspace_bytes": (c_size_t, [POINTER(WgradJob), c_int, c_int]),
    "sl_conv1d_wgrad_multi": (c_int, [POINTER(WgradJob), c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "sl_conv1d_wgrad_multi_plan": (c_int, [POINTER(WgradJob), c_int, c_int, POINTER(c_int), POINTER(c_int)]),
    "sl_pack_layers": (c_int, [c_void_p, POINTER(AdamLayer), c_int, c_int, c_void_p]),
    "sl_splitf16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_int64, c_int, c_void_p]),
    "sl_splitf16_pack_input": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_void_p]),
    "sl_wave_frames_planes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, c_float,
                                      c_int, c_void_p]),
    "sl_splitf16_pack_weights": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "sl_splitf16_adam_pack_layers": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(AdamLayer), c_int, c_int, c_float,
                                             c_float, c_float, c_float, c_float, c_void_p]),
    "sl_split3_wgrad_combine_scaled": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                               c_int, c_float, c_void_p]),
    "sl_splitf16_bias_grad": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64, c_float, c_void_p, c_size_t,
                                      c_void_p]),
    "sl_splitf16_dropout": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_float, ctypes.c_uint64, c_void_p]),
    "sl_grad_sqnorm_workspace_bytes": (c_size_t, [POINTER(NormRange), c_int]),
    "sl_grad_sqnorm": (c_int, [c_void_p, POINTER(NormRange), c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                               c_void_p]),
    "sl_clip_scale": (c_int, [c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    # the clipped twins: the original's arguments, then grad_scale (device float*, NULL = 1) and clipvalue (0 = off)
    "sl_adam_step_clipped": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_float, c_float, c_float,
                                     c_float, c_void_p, c_float, c_void_p]),
    "sl_adam_pack_layers_clipped": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(AdamLayer), c_int, c_int, c_int,
                                            c_float, c_float, c_float, c_float, c_void_p, c_float, c_void_p]),
    "sl_split3_adam_pack_layers_clipped": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(AdamLayer), c_int, c_int,
                                                   c_float, c_float, c_float, c_float, c_void_p, c_float, c_void_p]),
    "sl_splitf16_adam_pack_layers_clipped": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(AdamLayer), c_int, c_int,
                                                     c_float, c_float, c_float, c_float, c_float, c_void_p, c_float, c_void_p]),
    # the rules beside Adam: param, grad, s0, s1 (NULL for a one-slot rule), ..., rule, [w_scale,] grad_scale, clipvalue, stream
    "sl_optimizer_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, POINTER(OptRule), c_void_p, c_float,
                                  c_void_p]),
    "sl_optimizer_pack_layers": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(AdamLayer), c_int, c_int,
                                         POINTER(OptRule), c_void_p, c_float, c_void_p]),
    "sl_split3_optimizer_pack_layers": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(AdamLayer), c_int,
                                                POINTER(OptRule), c_void_p, c_float, c_void_p]),
    "sl_splitf16_optimizer_pack_layers": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(AdamLayer), c_int,
                                                  POINTER(OptRule), c_float, c_void_p, c_float, c_void_p]),
}


class HipLibrary:
    """Loaded libspeechless_hip.so with typed entry points.  `call(name, *args)` raises on a non-zero status."""

    def __init__(self, path=LIB_PATH):
        path = Path(path)
        if not path.exists():
            raise HipLibraryError(
                "{} not found: build it with `python -m speechless_amd.build` (or __graft_entry__.build()). "
                "The speechless_amd hot path has no CPU fallback.".format(path))
        self.path = path
        # PyDLL: the GIL is NOT released around a call.  Every entry point only enqueues work (microseconds); with CDLL
        # each of the ~60 launches of a step hands the GIL to the input pipeline's worker threads and has to win it back
        # (up to the interpreter's 5 ms switch interval) before the next launch can be issued.
        self._dll = ctypes.PyDLL(str(path)) if os.environ.get("SL_RELEASE_GIL", "0") != "1" else ctypes.CDLL(str(path))
        self._fn = {}
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(self._dll, name)  # AttributeError if the symbol is missing -> loud
            fn.restype = restype
            fn.argtypes = argtypes
            self._fn[name] = fn
        if self._fn["sl_version"]() != 1:
            raise HipLibraryError("libspeechless_hip.so version mismatch")

    def raw(self, name):
        return self._fn[name]

    def last_error(self):
        msg = self._fn["sl_last_error"]()
        return msg.decode("utf8", "replace") if msg else ""

    def call(self, name, *args):
        rc = self._fn[name](*args)
        if rc != 0:
            raise_status(name, rc, self.last_error)


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = HipLibrary()
    return _LIB
