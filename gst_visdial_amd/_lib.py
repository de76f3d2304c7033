"""ctypes binding of the C ABI declared in include/gstvd_hip.h (libgstvd_hip.so, gfx950).

There is NO fallback: if the shared library is missing or a call returns a non-zero status the
product raises.  (Build it with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C gst_visdial_amd/csrc`.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgstvd_hip.so")
ABI_VERSION = 9

F32, BF16 = 0, 1
F16 = 2                                # the in-domain filter's entries only
GAUSS_MAX_D, GAUSS_FIT_SLAB = 1024, 4096
COS_TOPK_AUTO, COS_TOPK_MANY, COS_TOPK_FEW = 0, 1, 2
EPI_BIAS, EPI_ADD, EPI_GELU, EPI_DGELU, EPI_DROPOUT = 1, 2, 4, 8, 16
EPI_COLSUM, EPI_COLSUM_ACC = 32, 64
EPI_ADAMW = 128
LN_RESID, LN_EMBED, LN_IMAGE = 0, 1, 2
RANK_MAX_OPTIONS = 128
GEN_EVAL, GEN_TEST, GEN_TRAIN_A, GEN_TRAIN_Q = range(4)
(RANK_N_SPARSE, RANK_N_GT_SKIPPED, RANK_N_NDCG, RANK_N_NDCG_EMPTY, RANK_N_REL_SKIPPED, RANK_N_CALLS, RANK_NDCG_SUM) = range(7)
RANK_HIST = 8
RANK_ACC_SLOTS = RANK_HIST + RANK_MAX_OPTIONS + 1

_vp, _i64, _i32, _f32, _u32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_uint32


class GemmDesc(C.Structure):
    _fields_ = [("A", _vp), ("B", _vp), ("C", _vp), ("bias", _vp), ("addend", _vp), ("aux", _vp),
                ("M", _i64), ("N", _i64), ("K", _i64),
                ("lda", _i64), ("ldb", _i64), ("ldc", _i64), ("ldadd", _i64), ("ldaux", _i64),
                ("batch", _i64), ("sA", _i64), ("sB", _i64), ("sC", _i64), ("sAdd", _i64), ("sAux", _i64),
                ("dtype_in", _i32), ("dtype_out", _i32), ("a_kmajor", _i32), ("b_kmajor", _i32), ("epilogue", _i32),
                ("alpha", _f32), ("dropout_p", _f32), ("site", _u32), ("rng", _vp)]


class LnDesc(C.Structure):
    _fields_ = [("mode", _i32), ("dtype", _i32), ("M", _i64), ("H", _i64),
                ("x", _vp), ("ldx", _i64), ("res", _vp), ("ldres", _i64),
                ("gamma", _vp), ("beta", _vp), ("eps", _f32),
                ("y", _vp), ("ldy", _i64), ("mean", _vp), ("rstd", _vp),
                ("p_pre", _f32), ("p_post", _f32), ("site_pre", _u32), ("site_post", _u32), ("rng", _vp),
                ("ids", _vp), ("segs", _vp), ("T", _i64), ("type_vocab", _i32),
                ("word", _vp), ("pos", _vp), ("tt", _vp), ("tt_ext", _vp),
                ("loc", _vp), ("w_loc", _vp), ("b_loc", _vp), ("pos_offset", _i64)]


class LnBwdDesc(C.Structure):
    _fields_ = [("f", LnDesc), ("dy", _vp), ("lddy", _i64), ("dres", _vp), ("lddres", _i64),
                ("dx", _vp), ("lddx", _i64), ("partial", _vp),
                ("dword", _vp), ("dpos", _vp), ("dtt", _vp), ("dtt_ext", _vp), ("nblk", _i64)]


class AttnDesc(C.Structure):
    _fields_ = [("Q", _vp), ("K", _vp), ("V", _vp), ("O", _vp), ("LSE", _vp), ("key_mask", _vp),
                ("ldq", _i64), ("ldk", _i64), ("ldv", _i64), ("ldo", _i64),
                ("B", _i32), ("nh", _i32), ("Lq", _i32), ("Lk", _i32), ("d", _i32), ("causal", _i32), ("dtype", _i32),
                ("mask_neg", _f32), ("scale", _f32), ("dropout_p", _f32), ("site", _u32), ("rng", _vp),
                ("dO", _vp), ("lddo", _i64), ("dQ", _vp), ("dK", _vp), ("dV", _vp),
                ("lddq", _i64), ("lddk", _i64), ("lddv", _i64), ("delta", _vp), ("kv_group", _i32),
                ("q_bstride", _i32), ("kv_bstride", _i32), ("drop_bits", _vp)]


class SampleDesc(C.Structure):
    _fields_ = [("logits", _vp), ("ld", _i64), ("dtype", _i32), ("B", _i32), ("V", _i32), ("top_k", _i32), ("temperature", _f32),
                ("u", _vp), ("out", _vp), ("out_stride", _i64), ("banned", _vp), ("banned_ld", _i64),
                ("hist", _vp), ("hist_ld", _i64), ("hist_T", _i32), ("ngram", _i32),
                ("ids_tm", _vp), ("ids_stride", _i64), ("cur_len", _i32), ("n_special", _i32), ("special", _i32 * 8),
                ("top_p", _f32), ("reserved_", _i32)]


class AdamFuse(C.Structure):
    """gstvd_adamw_fuse_t: the flat buffers and constants of the optimizer, for the weight-gradient launch that updates in its epilogue."""
    _fields_ = [("grad_base", _vp), ("param", _vp), ("m", _vp), ("v", _vp), ("shadow_bf16", _vp),
                ("step", _vp), ("beta1", _f32), ("beta2", _f32), ("eps", _f32), ("grad_scale", _f32), ("write_grad", _i32)]


class NspHeadDesc(C.Structure):
    """gstvd_nsp_head_t: first-token gather, poolers, fusion, bi_seq_relationship and the 2-way softmax of one launch."""
    _fields_ = [("xt", _vp), ("ldt", _i64), ("t_rows", _i64), ("xv", _vp), ("ldv", _i64), ("v_rows", _i64),
                ("wt", _vp), ("ldwt", _i64), ("wv", _vp), ("ldwv", _i64),
                ("bt", _vp), ("bv", _vp), ("wn", _vp), ("ldwn", _i64), ("bn", _vp),
                ("z", _vp), ("ldz", _i64), ("prob0", _vp),
                ("B", _i32), ("H", _i32), ("Hv", _i32), ("Hb", _i32), ("dtype", _i32), ("fusion", _i32),
                ("kernel_name", _vp), ("kernel_name_len", _i32), ("reserved_", _i32)]


class NspTrainDesc(C.Structure):
    """gstvd_nsp_train_t: the NSP head in training form -- forward with dropout, saved pt / pv / keep flags and the soft-label
    loss; backward down to the gradients in front of the two pooler ReLUs."""
    _fields_ = [("xt", _vp), ("ldt", _i64), ("t_rows", _i64), ("xv", _vp), ("ldv", _i64), ("v_rows", _i64),
                ("wt", _vp), ("ldwt", _i64), ("wv", _vp), ("ldwv", _i64),
                ("bt", _vp), ("bv", _vp), ("wn", _vp), ("ldwn", _i64), ("bn", _vp),
                ("labels", _vp), ("ldl", _i64),
                ("z", _vp), ("ldz", _i64),
                ("pt", _vp), ("pv", _vp), ("keep", _vp), ("row_loss", _vp), ("stats", _vp),
                ("gscale", _vp), ("dwn", _vp), ("lddwn", _i64), ("dbn", _vp), ("dpt", _vp), ("dpv", _vp), ("lddp", _i64),
                ("rng", _vp), ("p", _f32), ("site", _u32),
                ("B", _i32), ("H", _i32), ("Hv", _i32), ("Hb", _i32), ("dtype", _i32), ("fusion", _i32), ("acc_w", _i32), ("acc_b", _i32),
                ("kernel_name", _vp), ("kernel_name_len", _i32), ("reserved_", _i32)]


class BeamStepDesc(C.Structure):
    """gstvd_beam_step_t: one beam-search step -- the K best of the K x V continuations of every dialog row."""
    _fields_ = [("logits", _vp), ("ld", _i64), ("dtype", _i32), ("B", _i32), ("K", _i32), ("V", _i32),
                ("score_in", _vp), ("done_in", _vp), ("score_out", _vp), ("done_out", _vp), ("parent", _vp),
                ("ids_tm", _vp), ("ids_stride", _i64), ("positions", _i32), ("pos", _i32),
                ("workspace", _vp), ("eos", _i32), ("pad", _i32)]


class BeamReorderDesc(C.Structure):
    """gstvd_beam_reorder_t: the K | V columns of the surviving beams' self-attention caches, every decoder layer in one launch."""
    _fields_ = [("src", _vp * 16), ("dst", _vp * 16), ("parent", _vp), ("row_stride", _i64), ("ld", _i64),
                ("n_layers", _i32), ("B", _i32), ("K", _i32), ("H", _i32), ("Umax", _i32), ("t", _i32), ("dtype", _i32),
                ("reserved_", _i32)]


class ContextAppendDesc(C.Structure):
    """gstvd_context_append_t: the context splice of the generation loop for all rows in one launch."""
    _fields_ = [("ctx_ids", _vp), ("ld_ctx", _i64), ("segments", _vp), ("ld_seg", _i64), ("att_mask", _vp), ("ld_att", _i64),
                ("ctx_len", _vp), ("new_ids", _vp), ("ld_new", _i64), ("B", _i64), ("T", _i64), ("U", _i64),
                ("sep_id", _i64), ("segment_value", _i64), ("n_out", _vp), ("abnormal", _vp), ("full", _vp)]


class DialogRowsDesc(C.Structure):
    """gstvd_dialog_rows_t: the student's train rows of B generated dialogs of R rounds, one launch."""
    _fields_ = [("cap", _vp), ("ld_cap", _i64), ("ques", _vp), ("ans", _vp), ("ld_utt", _i64), ("ppl", _vp), ("valid", _vp),
                ("u_tok", _vp), ("ld_u", _i64),
                ("enc_ids", _vp), ("enc_seg", _vp), ("enc_mlm", _vp), ("enc_att", _vp), ("ld_enc", _i64),
                ("enc_sep", _vp), ("ld_sep", _i64), ("enc_hist_len", _vp),
                ("dec_ids", _vp), ("dec_labels", _vp), ("dec_att", _vp), ("ld_dec", _i64),
                ("mask_prob", C.c_double), ("threshold", C.c_double),
                ("cls", _i64), ("sep", _i64), ("mask", _i64), ("special", _i64 * 8),
                ("B", _i32), ("R", _i32), ("U", _i32), ("Lc", _i32), ("T", _i32), ("S", _i32), ("Ud", _i32), ("n_special", _i32),
                ("select_data", _i32), ("reserved_", _i32)]


class SubseqReplaceDesc(C.Structure):
    """gstvd_subseq_replace_t: id-level substitutions inside one utterance of every context row, one launch."""
    _fields_ = [("ids", _vp), ("ld_ids", _i64), ("out_ids", _vp), ("ld_out", _i64), ("n_replaced", _vp),
                ("row_ptr", _vp), ("subs", _vp), ("pieces", _vp), ("cont", _vp), ("n_vocab", _i64),
                ("cls", _i64), ("sep", _i64), ("pad", _i64),
                ("segments", _vp), ("ld_seg", _i64), ("start_seg", _vp), ("ld_start", _i64),
                ("sep_indices", _vp), ("ld_sep", _i64), ("att_mask", _vp), ("ld_att", _i64),
                ("n", _i32), ("T", _i32), ("n_subs", _i32), ("n_pieces", _i32), ("max_sep", _i32), ("reserved_", _i32)]


class DiscRowsDesc(C.Structure):
    """gstvd_disc_rows_t: N rows of the discriminative model from token-id pools, one launch."""
    _fields_ = [("cap", _vp), ("ld_cap", _i64), ("ques", _vp), ("ans", _vp), ("ld_utt", _i64), ("opts", _vp), ("ld_opt", _i64),
                ("gt_index", _vp), ("dense_scores", _vp), ("row_dialog", _vp), ("row_round", _vp), ("row_slot", _vp),
                ("u_tok", _vp), ("ld_u", _i64), ("u_neg", _vp),
                ("tokens", _vp), ("segments", _vp), ("mask", _vp), ("att", _vp), ("ld_row", _i64),
                ("sep_indices", _vp), ("ld_sep", _i64), ("hist_len", _vp), ("neg_option", _vp), ("nsp_labels", _vp),
                ("mask_prob", C.c_double), ("cls", _i64), ("sep", _i64), ("mask_id", _i64), ("N", _i64),
                ("D", _i32), ("R", _i32), ("O", _i32), ("U", _i32), ("Lc", _i32), ("T", _i32), ("S", _i32),
                ("tot_rounds", _i32), ("num_options", _i32), ("train", _i32)]


class GenRowsDesc(C.Structure):
    """gstvd_gen_rows_t: encoder and decoder rows of the generative model from token-id pools, one launch."""
    _fields_ = [("cap", _vp), ("ld_cap", _i64), ("ques", _vp), ("ans", _vp), ("ld_utt", _i64), ("opts", _vp), ("ld_opt", _i64),
                ("gt_index", _vp), ("enc_dialog", _vp), ("enc_round", _vp), ("u_tok", _vp), ("ld_u", _i64),
                ("tokens", _vp), ("segments", _vp), ("mlm", _vp), ("att", _vp), ("ld_row", _i64),
                ("sep_indices", _vp), ("ld_sep", _i64), ("hist_len", _vp),
                ("dec_dialog", _vp), ("dec_round", _vp), ("dec_slot", _vp),
                ("dec_ids", _vp), ("dec_labels", _vp), ("dec_att", _vp), ("ld_dec", _i64), ("dec_option", _vp),
                ("mask_prob", C.c_double), ("cls", _i64), ("sep", _i64), ("mask_id", _i64), ("n_enc", _i64), ("n_dec", _i64),
                ("D", _i32), ("R", _i32), ("Ro", _i32), ("O", _i32), ("U", _i32), ("Lc", _i32), ("T", _i32), ("S", _i32), ("Ud", _i32),
                ("num_options", _i32), ("mode", _i32), ("reserved_", _i32)]


class RankMetricsDesc(C.Structure):
    """gstvd_rank_metrics_t: ranks, ground-truth ranks, NDCG ratios and accumulator additions of L score lists, one call."""
    _fields_ = [("scores", _vp), ("ld_scores", _i64), ("gt_index", _vp), ("relevance", _vp), ("ld_rel", _i64), ("n_rel", _i64),
                ("rel_index", _vp), ("discounts", _vp), ("n_discounts", _i64), ("ranks", _vp), ("ld_ranks", _i64),
                ("gt_rank", _vp), ("ndcg", _vp), ("acc", _vp), ("L", _i64), ("O", _i32), ("reserved_", _i32)]


class GaussFitDesc(C.Structure):
    """gstvd_gauss_fit_t: mean and covariance of N feature rows in float64, two launches."""
    _fields_ = [("x", _vp), ("ldx", _i64), ("N", _i64), ("mean", _vp), ("cov", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
                ("D", _i32), ("dtype", _i32)]


class GaussLogprobDesc(C.Structure):
    """gstvd_gauss_logprob_t: the Gaussian log density of M feature rows and the optional cut at a threshold, one launch."""
    _fields_ = [("x", _vp), ("ldx", _i64), ("M", _i64), ("mean", _vp), ("w_packed", _vp),
                ("klog2pi", C.c_double), ("half_log_det", C.c_double), ("threshold", C.c_double),
                ("out", _vp), ("keep", _vp), ("n_kept", _vp), ("D", _i32), ("dtype", _i32)]


class ColsumEntry(C.Structure):
    _fields_ = [("partial", _vp), ("out", _vp * 3), ("nblk", _i64), ("stride", _i64), ("H", _i64),
                ("nvec", _i32), ("accumulate", _i32 * 3), ("blk0", _i32)]


class SlabEntry(C.Structure):
    _fields_ = [("x", _vp), ("scratch", _vp), ("ldx", _i64), ("M", _i64), ("N", _i64), ("blk0", _i32), ("pad_", _i32)]


# name -> (restype, argtypes); every symbol include/gstvd_hip.h declares
SIGNATURES = {
    "gstvd_abi_version": (_i32, []),
    "gstvd_build_arch": (C.c_char_p, []),
    "gstvd_gemm": (_i32, [C.POINTER(GemmDesc), _vp]),
    "gstvd_gemm_splitk_ws_bytes": (_i64, [_i64, _i64, _i32]),
    "gstvd_gemm_splitk": (_i32, [_vp, _i32, _vp, _i64, _vp]),
    "gstvd_gemm_group_tile": (_i32, []),
    "gstvd_gemm_group_caps": (_i32, []),
    "gstvd_gemv_ln": (_i32, [C.POINTER(GemmDesc), _vp, _vp, _f32, _vp, _i64, _vp]),
    "gstvd_gemm_kernel_name": (_i32, [C.POINTER(GemmDesc), _i32, C.c_char_p, _i32]),
    "gstvd_gemm_grouped_kernel_name": (_i32, [_i32, _i32, _i32, _i32, C.c_char_p, _i32]),
    "gstvd_gemm_grouped": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    "gstvd_ln_fwd": (_i32, [C.POINTER(LnDesc), _vp]),
    "gstvd_ln_bwd_blocks": (_i64, [_i64]),
    "gstvd_ln_bwd_blocks_for": (_i64, [_i64, _i64, _i32]),
    "gstvd_ln_bwd": (_i32, [C.POINTER(LnBwdDesc), _vp]),
    "gstvd_gemm_ln_fwd": (_i32, [C.POINTER(GemmDesc), C.POINTER(LnDesc), _vp]),
    "gstvd_gemm_ln_bwd": (_i32, [C.POINTER(GemmDesc), C.POINTER(LnBwdDesc), _vp]),
    "gstvd_gemm_ln_rows_per_block": (_i64, []),
    "gstvd_colsum_partials": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i32, _vp]),
    "gstvd_colsum_batched": (_i32, [_vp, _i64, _i64, _vp]),
    "gstvd_colsum_slabs_batched": (_i32, [_vp, _i64, _i64, _i32, _vp]),
    "gstvd_colsum_slabs": (_i32, [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp]),
    "gstvd_colsum": (_i32, [_vp, _i64, _i64, _i64, _i32, _vp, _vp, _i64, _i32, _vp]),
    "gstvd_locgrad": (_i32, [_vp, _i64, _vp, _i64, _i64, _i32, _vp, _i32, _vp]),
    "gstvd_attn_fwd": (_i32, [C.POINTER(AttnDesc), _vp]),
    "gstvd_attn_bwd": (_i32, [C.POINTER(AttnDesc), _vp]),
    "gstvd_attn_group_bwd": (_i32, [C.POINTER(AttnDesc), _vp]),
    "gstvd_ln_kernel_name": (_i32, [_vp, _i32, C.c_char_p, _i32]),
    "gstvd_attn_kernel_name": (_i32, [C.POINTER(AttnDesc), _i32, C.c_char_p, _i32]),
    "gstvd_attn_probs": (_i32, [C.POINTER(AttnDesc), _vp, _i32, _vp]),
    "gstvd_ce_fwd": (_i32, [_vp, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "gstvd_ce_bwd": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _vp, _i64, _vp]),
    "gstvd_ce_bwd_rows": (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp]),
    "gstvd_fgsm_step": (_i32, [_vp, _vp, _f32, _vp, _i64, _vp]),
    "gstvd_answer_scores": (_i32, [_vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _vp]),
    "gstvd_rank_loss": (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gstvd_sample_topk": (_i32, [C.POINTER(SampleDesc), _vp]),
    "gstvd_sample_topk_scored": (_i32, [C.POINTER(SampleDesc), _vp, _i64, _vp]),
    "gstvd_vl_split": (_i32, [_vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _f32, _u32, _u32, _vp, _vp]),
    "gstvd_cast": (_i32, [_vp, _i32, _vp, _i32, _i64, _vp]),
    "gstvd_cast_ranges": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    "gstvd_scale": (_i32, [_vp, _vp, _i64, _vp]),
    "gstvd_rng_advance": (_i32, [_vp, _vp]),
    "gstvd_dropout_mask": (_i32, [_vp, _i64, _f32, _u32, _vp, _vp]),
    "gstvd_adamw": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _f32, _f32, _f32, _vp, _f32, _i64, _vp]),
    "gstvd_adamw_bf16grad": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _f32, _f32, _f32, _vp, _f32, _i64, _vp]),
    "gstvd_adamw_blocks": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _f32, _f32, _f32, _vp, _f32, _i64, _vp, _i64, _vp, _vp]),
    "gstvd_gemm_grouped_adamw": (_i32, [_vp, _vp, _i64, _i64, C.POINTER(AdamFuse), _vp, _i64, _vp]),
    "gstvd_gemm_grouped_adamw_kernel_name": (_i32, [C.c_char_p, _i32]),
    "gstvd_nsp_head": (_i32, [C.POINTER(NspHeadDesc), _vp]),
    "gstvd_rows_gather": (_i32, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp]),
    "gstvd_rows_scatter": (_i32, [_vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp]),
    "gstvd_rows_mul": (_i32, [_vp, _i64, _vp, _i64, _i64, _i64, _i32, _vp]),
    "gstvd_kl_fwd": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "gstvd_kl_bwd": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i32, _vp, _i64, _vp]),
    "gstvd_nsp_train_fwd": (_i32, [C.POINTER(NspTrainDesc), _vp]),
    "gstvd_nsp_train_bwd": (_i32, [C.POINTER(NspTrainDesc), _vp]),
    "gstvd_beam_step": (_i32, [C.POINTER(BeamStepDesc), _vp]),
    "gstvd_beam_reorder": (_i32, [C.POINTER(BeamReorderDesc), _vp]),
    "gstvd_context_append": (_i32, [C.POINTER(ContextAppendDesc), _vp]),
    "gstvd_dialog_rows": (_i32, [C.POINTER(DialogRowsDesc), _vp]),
    "gstvd_rows_argmax": (_i32, [_vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp]),
    "gstvd_vocab_argmax_ws_bytes": (_i64, [_i64, _i64]),
    "gstvd_vocab_argmax": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _vp]),
    "gstvd_topk_logp": (_i32, [_vp, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp]),
    "gstvd_distill_fwd": (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gstvd_cos_topk_route": (_i32, [_i64, _i64]),
    "gstvd_cos_topk_ws_bytes": (_i64, [_i64, _i64, _i32]),
    "gstvd_cos_topk": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i32, _f32, _i32, _vp, _i64, _vp, _vp, _vp]),
    "gstvd_subseq_replace": (_i32, [C.POINTER(SubseqReplaceDesc), _vp]),
    "gstvd_disc_rows": (_i32, [C.POINTER(DiscRowsDesc), _vp]),
    "gstvd_gen_rows": (_i32, [C.POINTER(GenRowsDesc), _vp]),
    "gstvd_rank_metrics": (_i32, [C.POINTER(RankMetricsDesc), _vp]),
    "gstvd_gauss_fit_ws_bytes": (_i64, [_i64, _i32]),
    "gstvd_gauss_fit": (_i32, [C.POINTER(GaussFitDesc), _vp]),
    "gstvd_gauss_w_packed_elems": (_i64, [_i32]),
    "gstvd_gauss_logprob": (_i32, [C.POINTER(GaussLogprobDesc), _vp]),
    "gstvd_distill_bwd": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _f32, _i32, _vp, _i64, _vp]),
}

_STATUS = {-1: "GSTVD_E_DTYPE", -2: "GSTVD_E_SHAPE", -3: "GSTVD_E_ALIGN", -4: "GSTVD_E_NULL", -5: "GSTVD_E_UNSUPPORTED"}


class GstvdError(RuntimeError):
    pass


_lib = None


def load():
    """Load libgstvd_hip.so (once).  Raises if it is missing -- there is no CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GstvdError(
            "gst_visdial_amd: HIP library %s not found; build it first (make -C gst_visdial_amd/csrc). "
            "There is no CPU fallback for the product path." % LIB_PATH)
    # torch first: its wheel bundles its own HIP runtime (libamdhip64).  If this library were dlopen'ed before torch, the
    # loader would pull in /opt/rocm's copy for it and torch would then bring a second runtime into the process -- kernels
    # registered with one, streams and allocations owned by the other (observed: hipErrorNoDevice on the first launch).
    # With torch loaded first the dependency resolves to the runtime already in the process.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.gstvd_abi_version() != ABI_VERSION:
        raise GstvdError("libgstvd_hip.so ABI %d != expected %d; rebuild" % (lib.gstvd_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


N_CALLS = [0]      # launching library calls made so far (each is >= 1 kernel launch): bench.py reports calls per decode token


def status_name(rc):
    """The name of an entry point's return value: "ok", a GSTVD_E_* name, or the hipError_t of the launch."""
    if rc == 0:
        return "ok"
    return _STATUS.get(rc, "hipError_t %d" % rc if rc > 0 else "status %d" % rc)


def check(name, rc):
    N_CALLS[0] += 1
    if rc != 0:
        raise GstvdError("%s failed: %s" % (name, status_name(rc)))
