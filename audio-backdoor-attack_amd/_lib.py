"""ctypes binding of libabd.so (the C ABI in include/abd.h).

The library is built in-tree (``make -C audio-backdoor-attack_amd``).  There is no
fallback: if the .so is missing or no HIP device is present, every compute entry
point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ABD_LIB", os.path.join(HERE, "libabd.so"))

ABD_MEL_HTK, ABD_MEL_SLANEY = 0, 1
ABD_PAD_REFLECT, ABD_PAD_CONSTANT = 0, 1
INJECT_NONE, INJECT_ADD, INJECT_SNR_WINDOW, INJECT_HALF_MIX, INJECT_DEPLOY, INJECT_DEPLOY_CLAMP = 0, 1, 2, 3, 4, 5
MFCC_INFO = {"fast": 0, "ppb": 1, "chunks": 2, "mel_path": 3, "dct_kernel": 4, "bwd_ok": 5}   # ABD_MFCC_INFO_*
MFCC_MEL_PATHS = ("generic", "half_slot", "segmented", "blue_slots")                           # ABD_MFCC_MEL_*
MFCC_DCT_KERNELS = ("plain", "lds", "mfma1", "mfma2", "mfma3")                                 # ABD_MFCC_DCT_*
METRICS_WORDS = 8

EXPORTS = (
    "abd_last_error", "abd_version",
    "abd_mfcc_plan_create", "abd_mfcc_plan_destroy", "abd_mfcc_plan_frames", "abd_mfcc_plan_describe",
    "abd_mfcc_plan_info",
    "abd_mfcc_workspace_bytes", "abd_mfcc_f32", "abd_mfcc_rows_f32", "abd_gather_rows_f32", "abd_inject_waveform_f32", "abd_inject_workspace_bytes",
    "abd_inject_row_scales",
    "abd_pydub_overlay_i16", "abd_mfcc_deploy_backward_workspace_bytes", "abd_mfcc_deploy_backward",
    "abd_smallcnn_create", "abd_smallcnn_destroy", "abd_smallcnn_param_count", "abd_smallcnn_param_offsets",
    "abd_smallcnn_flat_features", "abd_smallcnn_workspace_bytes", "abd_smallcnn_workspace_offset", "abd_smallcnn_bn1_folded", "abd_smallcnn_conv2_planes",
    "abd_smallcnn_train_step",
    "abd_smallcnn_apply", "abd_smallcnn_forward", "abd_smallcnn_backward", "abd_smallcnn_eval", "abd_adam_f32",
    "abd_smallcnn_input_grad_workspace_bytes", "abd_smallcnn_input_grad",
    "abd_smallcnn_ablate_workspace_bytes", "abd_smallcnn_ablate_eval",
    "abd_segment_norms_workspace_bytes", "abd_segment_norms_f32", "abd_perturb_f32", "abd_sgd_f32",
    "abd_smallcnn_finetune_reg_workspace_bytes", "abd_smallcnn_finetune_reg_step",
    "abd_row_abs_sums_f32", "abd_smallcnn_unlearn_workspace_bytes", "abd_smallcnn_unlearn_step",
    "abd_reinit_weights_f32", "abd_smallcnn_unlearn_run", "abd_nwc_pair_f32",
    "abd_smallcnn_hidden_sums", "abd_smallcnn_fcprune_workspace_bytes", "abd_smallcnn_fcprune_eval",
    "abd_smallcnn_pruned_finetune_workspace_bytes", "abd_smallcnn_pruned_finetune_step",
    "abd_lstmattn_create", "abd_lstmattn_destroy", "abd_lstmattn_param_count", "abd_lstmattn_param_offsets",
    "abd_lstmattn_tile_rows", "abd_lstmattn_workspace_bytes", "abd_lstmattn_workspace_offset", "abd_lstmattn_forward",
    "abd_lstmattn_backward", "abd_lstmattn_train_step", "abd_lstmattn_eval",
    "abd_per_utterance_lstmattn_workspace_bytes", "abd_per_utterance_lstmattn_forward",
    "abd_rnn_create", "abd_rnn_destroy", "abd_rnn_param_count", "abd_rnn_param_offsets", "abd_rnn_tile_info",
    "abd_rnn_workspace_bytes", "abd_rnn_workspace_offset", "abd_rnn_forward", "abd_rnn_backward",
    "abd_rnn_train_step", "abd_rnn_eval",
    "abd_largecnn_create", "abd_largecnn_destroy", "abd_largecnn_param_count", "abd_largecnn_param_offsets",
    "abd_largecnn_tile_info", "abd_largecnn_linear_features", "abd_largecnn_workspace_bytes",
    "abd_largecnn_workspace_offset", "abd_largecnn_set_large_min_blocks", "abd_largecnn_forward",
    "abd_largecnn_backward", "abd_largecnn_train_step", "abd_largecnn_eval",
    "abd_resnet_create", "abd_resnet_destroy", "abd_resnet_param_count", "abd_resnet_param_offsets",
    "abd_resnet_running_count", "abd_resnet_running_offsets", "abd_resnet_tile_info", "abd_resnet_linear_features",
    "abd_resnet_workspace_bytes", "abd_resnet_workspace_offset", "abd_resnet_forward", "abd_resnet_backward",
    "abd_resnet_train_step", "abd_resnet_eval",
    "abd_smalllstm_create", "abd_smalllstm_destroy", "abd_smalllstm_param_count", "abd_smalllstm_param_offsets",
    "abd_smalllstm_running_count", "abd_smalllstm_running_offsets", "abd_smalllstm_tile_info",
    "abd_smalllstm_rnn_features", "abd_smalllstm_workspace_bytes", "abd_smalllstm_workspace_offset",
    "abd_smalllstm_forward", "abd_smalllstm_backward", "abd_smalllstm_train_step", "abd_smalllstm_eval",
    "abd_profile_start", "abd_profile_start_every", "abd_profile_step", "abd_profile_stop",
)

# csrc/prof.h phase ids
PHASES = ("stft_mel", "db_dct", "row_scale", "prep_weights", "conv1_stats", "conv1_bn_pool", "conv2_fwd",
          "bn2_pool", "conv3_fwd", "bn3_pool_dropout", "fc1_fwd", "fc2_loss", "metrics", "fc2_bwd", "fc1_wgrad",
          "fc1_dgrad", "bn3_bwd", "conv3_wgrad", "conv3_dgrad", "bn2_bwd", "conv2_wgrad", "conv2_dgrad",
          "conv1_bwd_wgrad", "adam", "finalize", "head_fwd", "head_mid", "head_bwd", "head_dgrad",
          "feat_gather")


class Inject(C.Structure):
    _fields_ = [
        ("mode", C.c_int),
        ("trigger", C.c_void_p),
        ("trigger_len", C.c_int64),
        ("poison", C.c_void_p),
        ("position", C.c_void_p),
        ("snr_db", C.c_float),
        ("patch", C.c_int),
        ("patch_t0", C.c_int), ("patch_t1", C.c_int), ("patch_c0", C.c_int), ("patch_c1", C.c_int),
        ("patch_value", C.c_float),
        ("frames", C.c_void_p), ("frame_pad", C.c_float),
        ("row_scale", C.c_void_p),
    ]


class Effect(C.Structure):
    _fields_ = [("kind", C.c_int), ("p", C.c_float * 8)]


FX_GAIN, FX_DISTORTION, FX_LADDER, FX_PHASER, FX_CHORUS, FX_REVERB, FX_PITCHSHIFT = 0, 1, 2, 3, 4, 5, 6
PREC_F32, PREC_BF16, PREC_F32_SPLIT = 0, 1, 2
PRECISIONS = {"f32": PREC_F32, "bf16": PREC_BF16, "f32split": PREC_F32_SPLIT}
ABLATE_CONV_FILTER, ABLATE_BN_WEIGHT = 0, 1
ABLATE_KINDS = {"conv": ABLATE_CONV_FILTER, "bn": ABLATE_BN_WEIGHT}
ABLATE_CHANNELS = 160   # mask columns: conv1 0..63, conv2 64..127, conv3 128..159


class TrainArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("labels", C.c_void_p), ("indicators", C.c_void_p), ("batch", C.c_int64),
        ("params", C.c_void_p), ("grads", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
        ("running", C.c_void_p), ("adam_step", C.c_int64),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("do_update", C.c_int),
        ("mask1_in", C.c_void_p), ("mask2_in", C.c_void_p), ("seed", C.c_uint64), ("counter", C.c_uint64),
        ("mask1_out", C.c_void_p), ("mask2_out", C.c_void_p), ("logprobs_out", C.c_void_p),
        ("metrics", C.c_void_p), ("grad_scale", C.c_float), ("num_batches_tracked", C.c_void_p),
        ("fc_grads_event", C.c_void_p), ("row_offset", C.c_int64),
        ("bn_sync_buf", C.c_void_p), ("bn_sync", C.c_void_p), ("bn_sync_ctx", C.c_void_p),
    ]


class LstmAttnArgs(C.Structure):
    """abd_lstmattn_args: abd_train_args without the second mask and the DP / SyncBN fields."""
    _fields_ = [
        ("x", C.c_void_p), ("labels", C.c_void_p), ("indicators", C.c_void_p), ("batch", C.c_int64),
        ("params", C.c_void_p), ("grads", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
        ("running", C.c_void_p), ("adam_step", C.c_int64),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("do_update", C.c_int),
        ("mask_in", C.c_void_p), ("seed", C.c_uint64), ("counter", C.c_uint64),
        ("mask_out", C.c_void_p), ("logits_out", C.c_void_p),
        ("metrics", C.c_void_p), ("grad_scale", C.c_float), ("num_batches_tracked", C.c_void_p),
        ("row_offset", C.c_int64),
    ]


class RnnArgs(C.Structure):
    """abd_rnn_args: abd_lstmattn_args without the dropout and running-statistics fields."""
    _fields_ = [
        ("x", C.c_void_p), ("labels", C.c_void_p), ("indicators", C.c_void_p), ("batch", C.c_int64),
        ("params", C.c_void_p), ("grads", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
        ("adam_step", C.c_int64),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("do_update", C.c_int),
        ("logits_out", C.c_void_p), ("metrics", C.c_void_p), ("grad_scale", C.c_float),
    ]


class LargeCnnArgs(C.Structure):
    """abd_largecnn_args: abd_rnn_args plus the two dropout masks, their seed / counter and the row offset."""
    _fields_ = [
        ("x", C.c_void_p), ("labels", C.c_void_p), ("indicators", C.c_void_p), ("batch", C.c_int64),
        ("params", C.c_void_p), ("grads", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
        ("adam_step", C.c_int64),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("do_update", C.c_int),
        ("mask1_in", C.c_void_p), ("mask2_in", C.c_void_p), ("seed", C.c_uint64), ("counter", C.c_uint64),
        ("mask1_out", C.c_void_p), ("mask2_out", C.c_void_p),
        ("logits_out", C.c_void_p), ("metrics", C.c_void_p), ("grad_scale", C.c_float), ("row_offset", C.c_int64),
    ]


class ResNetArgs(C.Structure):
    """abd_resnet_args: abd_rnn_args plus the running statistics and num_batches_tracked."""
    _fields_ = [
        ("x", C.c_void_p), ("labels", C.c_void_p), ("indicators", C.c_void_p), ("batch", C.c_int64),
        ("params", C.c_void_p), ("grads", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
        ("running", C.c_void_p), ("adam_step", C.c_int64),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("do_update", C.c_int),
        ("logits_out", C.c_void_p), ("metrics", C.c_void_p), ("grad_scale", C.c_float),
        ("num_batches_tracked", C.c_void_p),
    ]


class SmallLstmArgs(C.Structure):
    """abd_smalllstm_args: the fields of abd_lstmattn_args (one dropout mask, the running statistics)."""
    _fields_ = list(LstmAttnArgs._fields_)


class FinetuneRegArgs(C.Structure):
    """abd_finetune_reg_args: one batch of train_finetuning_reg (ft_reg.py:83-123)."""
    _fields_ = [
        ("x", C.c_void_p), ("labels", C.c_void_p), ("batch", C.c_int64),
        ("params", C.c_void_p), ("grads", C.c_void_p), ("running", C.c_void_p), ("num_batches_tracked", C.c_void_p),
        ("seed", C.c_uint64), ("counter", C.c_uint64), ("row_offset", C.c_int64),
        ("r", C.c_float), ("alpha", C.c_float), ("lr", C.c_float), ("momentum", C.c_float),
        ("momentum_buf", C.c_void_p),
        ("mask1_in", C.c_void_p * 3), ("mask2_in", C.c_void_p * 3),
        ("mask1_out", C.c_void_p * 3), ("mask2_out", C.c_void_p * 3),
        ("logprobs_out", C.c_void_p), ("loss_sum", C.c_void_p), ("correct", C.c_void_p),
    ]


MAX_SEGMENTS = 32


class RowSegment(C.Structure):
    """abd_row_segment: `rows` rows of `row_len` floats from element `offset` of a flat buffer."""
    _fields_ = [("offset", C.c_int64), ("rows", C.c_int64), ("row_len", C.c_int64)]


class UnlearnArgs(C.Structure):
    """abd_unlearn_args: one batch of train_unlearning (tsbd.py:108-138)."""
    _fields_ = [
        ("x", C.c_void_p), ("labels", C.c_void_p), ("batch", C.c_int64),
        ("params", C.c_void_p), ("grads", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
        ("running", C.c_void_p), ("num_batches_tracked", C.c_void_p),
        ("adam_step", C.c_int64), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("seed", C.c_uint64), ("counter", C.c_uint64), ("row_offset", C.c_int64),
        ("mask1_in", C.c_void_p), ("mask2_in", C.c_void_p), ("mask1_out", C.c_void_p), ("mask2_out", C.c_void_p),
        ("logprobs_out", C.c_void_p), ("metrics", C.c_void_p),
        ("record_offset", C.c_int64), ("record_rows", C.c_int64), ("record_row_len", C.c_int64),
        ("record_abs_sums", C.c_void_p),
    ]


MAX_REINIT_VARIANTS = 16
MAX_REINIT_ROWS = 1024
NWC_STATS_WORDS = 9   # abd_nwc_pair_f32's stats: n, mean_x, mean_y, sxx, syy, sxy, r, slope, intercept


class PrunedFinetuneArgs(C.Structure):
    """abd_pruned_finetune_args: one batch of train_finetuning under prune.custom_from_mask (fp.py:52-76)."""
    _fields_ = [
        ("x", C.c_void_p), ("labels", C.c_void_p), ("batch", C.c_int64),
        ("params", C.c_void_p), ("grads", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
        ("running", C.c_void_p), ("num_batches_tracked", C.c_void_p), ("pruned", C.c_void_p),
        ("adam_step", C.c_int64), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("seed", C.c_uint64), ("counter", C.c_uint64), ("row_offset", C.c_int64),
        ("mask1_in", C.c_void_p), ("mask2_in", C.c_void_p), ("mask1_out", C.c_void_p), ("mask2_out", C.c_void_p),
        ("logprobs_out", C.c_void_p), ("metrics", C.c_void_p),
    ]


FCPRUNE_UNITS = 128            # fc2's inputs: the units fp.py ranks and prunes
FCPRUNE_PASS_VARIANTS = 128    # variants whose masks one launch carries as kernel arguments


# int (*bn_sync)(void* ctx, int point, int64_t offset, int64_t n)  (abd_train_args.bn_sync)
BN_SYNC_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int64)
BN_SYNC_STRIDE = 136


class AbdError(RuntimeError):
    pass


_lock = threading.Lock()
_lib = None


def _declare(lib):
    vp, i64, i32, f32, sz = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_size_t
    sig = {
        "abd_last_error": (C.c_char_p, []),
        "abd_version": (i32, []),
        "abd_mfcc_plan_create": (i32, [i32, i32, i32, i32, i32, i32, i32, f32, i64, C.POINTER(vp)]),
        "abd_mfcc_plan_destroy": (None, [vp]),
        "abd_mfcc_plan_frames": (i32, [vp]),
        "abd_mfcc_plan_describe": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "abd_mfcc_plan_info": (i32, [vp, i32]),
        "abd_mfcc_workspace_bytes": (sz, [vp, i64]),
        "abd_mfcc_f32": (i32, [vp, vp, i64, vp, i64, C.POINTER(Inject), vp, vp, sz, vp]),
        "abd_mfcc_rows_f32": (i32, [vp, vp, i64, vp, i64, C.POINTER(Inject), vp, vp, vp, sz, vp]),
        "abd_gather_rows_f32": (i32, [vp, i64, vp, i64, vp, vp]),
        "abd_inject_waveform_f32": (i32, [vp, i64, i64, vp, i64, C.POINTER(Inject), vp, vp, sz, vp]),
        "abd_inject_workspace_bytes": (sz, [i64]),
        "abd_inject_row_scales": (i32, [vp, i64, i64, i64, C.POINTER(Inject), vp, vp]),
        "abd_pydub_overlay_i16": (i32, [vp, i64, vp, i64, vp, i64, vp, vp]),
        "abd_pydub_overlay_ragged_i16": (i32, [vp, i64, vp, vp, i64, i64, vp, i64, i64, vp, vp, vp]),
        "abd_softmax_entropy": (i32, [vp, i64, i32, vp, vp, vp]),
        "abd_style_board_create": (i32, [C.POINTER(Effect), i32, i32, i64, C.POINTER(vp)]),
        "abd_style_board_destroy": (None, [vp]),
        "abd_style_board_apply": (i32, [vp, vp, i64, vp, i64, i64, vp, i64, vp, sz, vp]),
        "abd_style_board_workspace_bytes": (sz, [vp, i64]),
        "abd_resample_plan_create": (i32, [i32, i32, i32, C.c_double, C.POINTER(vp)]),
        "abd_resample_plan_destroy": (None, [vp]),
        "abd_resample_output_length": (i64, [vp, i64]),
        "abd_resample_f32": (i32, [vp, vp, i64, i64, i64, vp, i64, vp]),
        "abd_pair_cross_entropy": (i32, [vp, vp, i64, i32, vp, vp]),
        "abd_smallcnn_forward_per_utterance_workspace_bytes": (sz, [vp, i64]),
        "abd_smallcnn_forward_per_utterance": (i32, [vp, vp, i64, vp, C.c_uint64, C.c_uint64, vp, vp, vp, vp, sz,
                                                     vp]),
        "abd_mfcc_deploy_backward_workspace_bytes": (sz, [vp, i64, i64]),
        "abd_mfcc_deploy_backward": (i32, [vp, vp, i64, vp, i64, C.POINTER(Inject), vp, vp, i32, vp, sz, vp]),
        "abd_smallcnn_create": (i32, [i32, i32, i32, i32, C.POINTER(vp)]),
        "abd_smallcnn_destroy": (None, [vp]),
        "abd_smallcnn_set_precision": (i32, [vp, i32]),
        "abd_smallcnn_param_count": (i64, [vp]),
        "abd_smallcnn_param_offsets": (i32, [vp, C.POINTER(i64)]),
        "abd_smallcnn_flat_features": (i32, [vp]),
        "abd_smallcnn_workspace_bytes": (sz, [vp, i64]),
        "abd_smallcnn_workspace_offset": (i64, [vp, i64, C.c_char_p]),
        "abd_smallcnn_bn1_folded": (C.c_int, [vp, i64]),
        "abd_smallcnn_conv2_planes": (C.c_int, [vp, i64]),
        "abd_smallcnn_train_step": (i32, [vp, C.POINTER(TrainArgs), vp, sz, vp]),
        "abd_smallcnn_apply": (i32, [vp, C.POINTER(TrainArgs), vp, sz, vp]),
        "abd_smallcnn_forward": (i32, [vp, C.POINTER(TrainArgs), i32, vp, sz, vp]),
        "abd_smallcnn_backward": (i32, [vp, C.POINTER(TrainArgs), vp, vp, sz, vp]),
        "abd_smallcnn_eval": (i32, [vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "abd_adam_f32": (i32, [vp, vp, vp, vp, i64, i64, f32, f32, f32, f32, vp]),
        "abd_smallcnn_input_grad_workspace_bytes": (sz, [vp, i64]),
        "abd_smallcnn_input_grad": (i32, [vp, vp, i64, vp, vp, vp, f32, vp, vp, vp, vp, sz, vp]),
        "abd_smallcnn_ablate_workspace_bytes": (sz, [vp, i64, i32]),
        "abd_smallcnn_ablate_eval": (i32, [vp, vp, i64, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, sz, vp]),
        "abd_segment_norms_workspace_bytes": (sz, [C.POINTER(i64), i32]),
        "abd_segment_norms_f32": (i32, [vp, C.POINTER(i64), i32, vp, vp, sz, vp]),
        "abd_perturb_f32": (i32, [vp, vp, vp, C.POINTER(i64), i32, f32, vp, vp]),
        "abd_sgd_f32": (i32, [vp, vp, vp, f32, vp, f32, f32, vp, i64, vp]),
        "abd_smallcnn_finetune_reg_workspace_bytes": (sz, [vp, i64]),
        "abd_smallcnn_finetune_reg_step": (i32, [vp, C.POINTER(FinetuneRegArgs), vp, sz, vp]),
        "abd_row_abs_sums_f32": (i32, [vp, vp, C.POINTER(RowSegment), i32, vp, vp, vp]),
        "abd_smallcnn_unlearn_workspace_bytes": (sz, [vp, i64]),
        "abd_smallcnn_unlearn_step": (i32, [vp, C.POINTER(UnlearnArgs), vp, sz, vp]),
        "abd_reinit_weights_f32": (i32, [vp, i64, vp, C.POINTER(RowSegment), i32, vp, C.POINTER(i64), i32, vp, vp, vp,
                                         vp]),
        "abd_smallcnn_unlearn_run": (i32, [vp, C.POINTER(UnlearnArgs), i64, vp, sz, vp]),
        "abd_nwc_pair_f32": (i32, [vp, vp, vp, C.POINTER(RowSegment), i32, vp, vp, vp, vp, vp, vp, vp]),
        "abd_smallcnn_hidden_sums": (i32, [vp, vp, i64, vp, vp, vp, vp, sz, vp]),
        "abd_smallcnn_fcprune_workspace_bytes": (sz, [vp, i64, i32]),
        "abd_smallcnn_fcprune_eval": (i32, [vp, vp, i64, vp, vp, vp, vp, i32, vp, vp, vp, sz, vp]),
        "abd_smallcnn_pruned_finetune_workspace_bytes": (sz, [vp, i64]),
        "abd_smallcnn_pruned_finetune_step": (i32, [vp, C.POINTER(PrunedFinetuneArgs), vp, sz, vp]),
        "abd_lstmattn_create": (i32, [i32, i32, i32, C.POINTER(vp)]),
        "abd_lstmattn_destroy": (None, [vp]),
        "abd_lstmattn_param_count": (i64, [vp]),
        "abd_lstmattn_param_offsets": (i32, [vp, C.POINTER(i64)]),
        "abd_lstmattn_tile_rows": (i32, []),
        "abd_lstmattn_workspace_bytes": (sz, [vp, i64]),
        "abd_lstmattn_workspace_offset": (i64, [vp, i64, C.c_char_p]),
        "abd_lstmattn_forward": (i32, [vp, C.POINTER(LstmAttnArgs), i32, vp, sz, vp]),
        "abd_lstmattn_backward": (i32, [vp, C.POINTER(LstmAttnArgs), vp, vp, sz, vp]),
        "abd_lstmattn_train_step": (i32, [vp, C.POINTER(LstmAttnArgs), vp, sz, vp]),
        "abd_lstmattn_eval": (i32, [vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "abd_per_utterance_lstmattn_workspace_bytes": (sz, [vp, i64]),
        "abd_per_utterance_lstmattn_forward": (i32, [vp, vp, i64, vp, C.c_uint64, C.c_uint64, vp, vp, vp, sz, vp]),
        "abd_rnn_create": (i32, [i32, i32, i32, C.POINTER(vp)]),
        "abd_rnn_destroy": (None, [vp]),
        "abd_rnn_param_count": (i64, [vp]),
        "abd_rnn_param_offsets": (i32, [vp, C.POINTER(i64)]),
        "abd_rnn_tile_info": (i32, [i32]),
        "abd_rnn_workspace_bytes": (sz, [vp, i64]),
        "abd_rnn_workspace_offset": (i64, [vp, i64, C.c_char_p]),
        "abd_rnn_forward": (i32, [vp, C.POINTER(RnnArgs), vp, sz, vp]),
        "abd_rnn_backward": (i32, [vp, C.POINTER(RnnArgs), vp, vp, sz, vp]),
        "abd_rnn_train_step": (i32, [vp, C.POINTER(RnnArgs), vp, sz, vp]),
        "abd_rnn_eval": (i32, [vp, vp, i64, vp, vp, vp, vp, vp, vp, sz, vp]),
        "abd_largecnn_create": (i32, [i32, i32, i32, C.POINTER(vp)]),
        "abd_largecnn_destroy": (None, [vp]),
        "abd_largecnn_set_large_min_blocks": (i32, [vp, i32]),
        "abd_largecnn_param_count": (i64, [vp]),
        "abd_largecnn_param_offsets": (i32, [vp, C.POINTER(i64)]),
        "abd_largecnn_tile_info": (i32, [i32]),
        "abd_largecnn_linear_features": (i64, [i32, i32]),
        "abd_largecnn_workspace_bytes": (sz, [vp, i64]),
        "abd_largecnn_workspace_offset": (i64, [vp, i64, C.c_char_p]),
        "abd_largecnn_forward": (i32, [vp, C.POINTER(LargeCnnArgs), i32, vp, sz, vp]),
        "abd_largecnn_backward": (i32, [vp, C.POINTER(LargeCnnArgs), vp, vp, sz, vp]),
        "abd_largecnn_train_step": (i32, [vp, C.POINTER(LargeCnnArgs), vp, sz, vp]),
        "abd_largecnn_eval": (i32, [vp, vp, i64, vp, vp, vp, vp, vp, vp, sz, vp]),
        "abd_resnet_create": (i32, [i32, i32, i32, C.POINTER(vp)]),
        "abd_resnet_destroy": (None, [vp]),
        "abd_resnet_param_count": (i64, [vp]),
        "abd_resnet_param_offsets": (i32, [vp, C.POINTER(i64)]),
        "abd_resnet_running_count": (i64, [vp]),
        "abd_resnet_running_offsets": (i32, [vp, C.POINTER(i64)]),
        "abd_resnet_tile_info": (i32, [i32]),
        "abd_resnet_linear_features": (i64, [i32, i32]),
        "abd_resnet_workspace_bytes": (sz, [vp, i64]),
        "abd_resnet_workspace_offset": (i64, [vp, i64, C.c_char_p]),
        "abd_resnet_forward": (i32, [vp, C.POINTER(ResNetArgs), i32, vp, sz, vp]),
        "abd_resnet_backward": (i32, [vp, C.POINTER(ResNetArgs), vp, vp, sz, vp]),
        "abd_resnet_train_step": (i32, [vp, C.POINTER(ResNetArgs), vp, sz, vp]),
        "abd_resnet_eval": (i32, [vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "abd_smalllstm_create": (i32, [i32, i32, i32, C.POINTER(vp)]),
        "abd_smalllstm_destroy": (None, [vp]),
        "abd_smalllstm_param_count": (i64, [vp]),
        "abd_smalllstm_param_offsets": (i32, [vp, C.POINTER(i64)]),
        "abd_smalllstm_running_count": (i64, [vp]),
        "abd_smalllstm_running_offsets": (i32, [vp, C.POINTER(i64)]),
        "abd_smalllstm_tile_info": (i32, [i32]),
        "abd_smalllstm_rnn_features": (i64, [i32, i32]),
        "abd_smalllstm_workspace_bytes": (sz, [vp, i64]),
        "abd_smalllstm_workspace_offset": (i64, [vp, i64, C.c_char_p]),
        "abd_smalllstm_forward": (i32, [vp, C.POINTER(SmallLstmArgs), i32, vp, sz, vp]),
        "abd_smalllstm_backward": (i32, [vp, C.POINTER(SmallLstmArgs), vp, vp, sz, vp]),
        "abd_smalllstm_train_step": (i32, [vp, C.POINTER(SmallLstmArgs), vp, sz, vp]),
        "abd_smalllstm_eval": (i32, [vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "abd_profile_start": (i32, [C.c_ulonglong, i32]),
        "abd_profile_start_every": (i32, [C.c_ulonglong, i32, i32]),
        "abd_profile_step": (i32, []),
        "abd_profile_stop": (i32, [C.POINTER(C.c_double), C.POINTER(i32), i32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


def load_library(path: str | None = None):
    """Load (once) and return the ctypes handle.  Raises AbdError if the .so is absent."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise AbdError(f"libabd.so not found at {p}: build it with `make -C {HERE}` "
                           "(the HIP path has no CPU fallback)")
        lib = C.CDLL(p)
        _declare(lib)
        _lib = lib
        return lib


def lib():
    return _lib if _lib is not None else load_library()


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().abd_last_error().decode(errors="replace")
        raise AbdError(f"{what} failed (code {rc}): {msg}")


def stream_ptr(device=None) -> int:
    """The current torch HIP stream as a raw hipStream_t value (0 = legacy default)."""
    import torch
    return int(torch.cuda.current_stream(device).cuda_stream)


def require_device(t, what="tensor"):
    """HIP path only: refuse CPU tensors loudly (no silent fallback)."""
    if not t.is_cuda:
        raise AbdError(f"{what} must live on a ROCm/HIP device; the abd HIP path has no CPU fallback")
    if not t.is_contiguous():
        raise AbdError(f"{what} must be contiguous")


class PhaseProfiler:
    """HIP-event brackets recorded by libabd around the selected kernel launches."""

    def __init__(self, phases, max_records=4096, every=1):
        """every: bracket only every `every`-th launch of each phase (each bracket serialises the
        stream: ~4-5 us of idle GPU per event on MI355X); once `step()` is called, every launch of
        the phases inside every `every`-th STEP instead (no aliasing with a phase's launches per step)."""
        self.mask = 0
        for ph in phases:
            self.mask |= 1 << PHASES.index(ph)
        self.max_records = max_records
        self.every = int(every)

    def __enter__(self):
        check(lib().abd_profile_start_every(self.mask, self.max_records, self.every), "abd_profile_start_every")
        return self

    def step(self):
        """Mark the start of a step (abd_profile_step)."""
        check(lib().abd_profile_step(), "abd_profile_step")

    def __exit__(self, *exc):
        n = len(PHASES)
        ms = (C.c_double * n)()
        cnt = (C.c_int * n)()
        lib().abd_profile_stop(ms, cnt, n)
        self.result = {PHASES[i]: (ms[i], cnt[i]) for i in range(n) if cnt[i] > 0}
        return False
