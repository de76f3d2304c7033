// Self-training glue on the device: the context splice of the generation loop and the student's train rows of a generated dialog.
// Both are integer work on token ids that the reference does per row on the host (generate.py:145-160 / 214-228; the loader
// dataloader/dataloader_cc12m_gen.py:104-248 with utils/data_utils.py:34-71, which re-tokenises JSON text).  Here each is ONE launch
// without atomics, workspace or host synchronisation, so the ten-round loop and the row assembly run between graph replays with
// no host in between.  include/gstvd_hip.h states both rules in full.
//
//   context_append_kernel   one wave per dialog row: count the non-zero new ids (ballots), then the lanes copy the first n of them
//                           behind the row's context -- or lane 0 places the lone [SEP] of an overflowing row, or only the flags
//                           of a full one.
//   dialog_rows_kernel      one wave per output row (b, j): lane i owns utterance i of the round's context (caption, q0, a0, ..,
//                           qj: 2j + 2 <= 64 of them), an inclusive wave scan of len + 1 gives every utterance's separator
//                           position, each lane writes its tokens and its [SEP], all lanes zero the tail; the target row goes
//                           through a 64-entry LDS line (the answer without special ids).  Every output element is written once.
#include "common.h"

namespace {

constexpr int UMAX = 64;                                      // tokens of one utterance row (U, Lc <= 64: checked by the host entries)

__global__ __launch_bounds__(WAVE) void context_append_kernel(gstvd_context_append_t a) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x, T = a.T, U = a.U;
  const int64_t* nw = a.new_ids + b * a.ld_new;
  int64_t n = 0;
  for (int64_t c0 = 0; c0 < U; c0 += WAVE) {
    const int64_t c = c0 + lane;
    n += __popcll(__ballot(c < U && nw[c] != 0));
  }
  const int64_t start = a.ctx_len[b];                         // every lane reads it in front of lane 0's update below
  int64_t* ctx = a.ctx_ids + b * a.ld_ctx;
  int64_t n_eff;
  if (start >= 0 && start + n <= T) {
    n_eff = n;
    for (int64_t c = lane; c < n; c += WAVE) {
      const int64_t v = nw[c], p = start + c;
      ctx[p] = v;
      if (a.segments) a.segments[b * a.ld_seg + p] = a.segment_value;
      if (a.att_mask) a.att_mask[b * a.ld_att + p] = v != 0 ? 1.f : 0.f;
    }
  } else if (start >= 0 && start < T) {
    n_eff = 1;
    if (lane == 0) {
      ctx[start] = a.sep_id;
      if (a.segments) a.segments[b * a.ld_seg + start] = a.segment_value;
      if (a.att_mask) a.att_mask[b * a.ld_att + start] = a.sep_id != 0 ? 1.f : 0.f;
      a.abnormal[b] = 1;
    }
  } else {                                                    // full (or a length that is no length): flags only
    n_eff = 0;
    if (lane == 0) { a.abnormal[b] = 1; a.full[b] = 1; }
  }
  if (lane == 0) {
    if (n_eff) a.ctx_len[b] = start + n_eff;
    if (a.n_out) a.n_out[b] = n_eff;
  }
}

DEVFN bool is_special(const gstvd_dialog_rows_t& a, int64_t v) {
  bool s = false;
#pragma unroll
  for (int i = 0; i < 8; ++i) s = s || (i < a.n_special && a.special[i] == v);
  return s;
}

__global__ __launch_bounds__(WAVE) void dialog_rows_kernel(gstvd_dialog_rows_t a) {
  __shared__ int64_t ans_line[UMAX];
  const int lane = threadIdx.x;
  const int R = a.R, U = a.U, T = a.T, S = a.S, Ud = a.Ud;
  const int64_t row = blockIdx.x, b = row / R;
  const int j = (int)(row - b * R);
  const int n_utt = 2 * j + 2;                                // caption, q0, a0, ..., qj

  // ---- lane i: utterance i, its length under the rule
  const int64_t* src = nullptr;
  int cap = 0, len = 0;
  const bool is_cap = lane == 0;
  if (lane < n_utt) {
    if (is_cap) { src = a.cap + b * a.ld_cap; cap = a.Lc; }
    else {
      const int k = (lane - 1) >> 1;
      src = ((lane & 1) ? a.ques : a.ans) + (b * R + k) * a.ld_utt;
      cap = U;
    }
    if (is_cap) { while (len < cap && src[len] != 0) ++len; }
    else { for (int c = 0; c < cap; ++c) len += is_special(a, src[c]) ? 0 : 1; }
  }
  // ---- inclusive scan of len + 1: the running position of utterance i's [SEP] (position 0 is [CLS])
  const int sep_pos = wave_scan_incl(lane < n_utt ? len + 1 : 0, lane);
  const int total = __shfl(sep_pos, WAVE - 1, WAVE) + 1;      // untruncated row length
  int64_t* e_ids = a.enc_ids + row * a.ld_enc;
  int64_t* e_seg = a.enc_seg + row * a.ld_enc;
  int64_t* e_mlm = a.enc_mlm + row * a.ld_enc;
  float* e_att = a.enc_att + row * a.ld_enc;
  if (lane == 0) {
    e_ids[0] = a.cls; e_seg[0] = 1; e_mlm[0] = -1; e_att[0] = a.cls != 0 ? 1.f : 0.f;
    a.enc_hist_len[row] = 2 * j + 1;
  }
  if (lane < n_utt) {
    const int64_t seg = 1 ^ (lane & 1);
    const float* u = a.u_tok ? a.u_tok + row * a.ld_u : nullptr;
    int p = sep_pos - len;                                    // first token of the utterance
    for (int c = 0; c < cap && p < T; ++c) {
      const int64_t v = src[c];
      if (is_cap ? (c >= len) : is_special(a, v)) continue;
      const bool masked = u != nullptr && (double)u[p] < a.mask_prob;
      const int64_t id = masked ? a.mask : v;
      e_ids[p] = id; e_seg[p] = seg; e_mlm[p] = masked ? v : -1; e_att[p] = id != 0 ? 1.f : 0.f;
      ++p;
    }
    if (sep_pos < T) { e_ids[sep_pos] = a.sep; e_seg[sep_pos] = seg; e_mlm[sep_pos] = -1; e_att[sep_pos] = a.sep != 0 ? 1.f : 0.f; }
  }
  for (int p = total + lane; p < T; p += WAVE) { e_ids[p] = 0; e_seg[p] = 0; e_mlm[p] = -1; e_att[p] = 0.f; }
  for (int s = lane; s < S; s += WAVE) a.enc_sep[row * a.ld_sep + s] = s < n_utt ? sep_pos : 0;   // s < n_utt <= 64: s is this lane

  // ---- the target: answer j without special ids, cut to Ud - 2 tokens
  const int64_t* ans = a.ans + row * a.ld_utt;
  const int64_t av = lane < U ? ans[lane] : 0;
  const bool keep = lane < U && !is_special(a, av);
  const uint64_t kept = __ballot(keep);
  const int rank = __popcll(kept & ((1ull << lane) - 1ull));
  int n = __popcll(kept);
  n = n < Ud - 2 ? n : Ud - 2;
  if (keep && rank < n) ans_line[rank] = av;
  __syncthreads();
  const bool zeroed = (a.select_data != 0 && (double)a.ppl[row] >= a.threshold) || (a.valid != nullptr && a.valid[b] == 0);
  for (int i = lane; i < Ud; i += WAVE) {
    // the row in front of [SEP] -> [PAD]: [CLS] answer [SEP] 0 ...
    const int64_t cur = i == 0 ? a.cls : i <= n ? ans_line[i - 1] : i == n + 1 ? a.sep : 0;
    const int i1 = i + 1;
    const int64_t nxt = i1 >= Ud ? 0 : i1 <= n ? ans_line[i1 - 1] : i1 == n + 1 ? a.sep : 0;
    a.dec_ids[row * a.ld_dec + i] = cur == a.sep ? 0 : cur;
    a.dec_att[row * a.ld_dec + i] = cur != 0 ? 1.f : 0.f;
    a.dec_labels[row * a.ld_dec + i] = zeroed ? 0 : nxt;
  }
}

}  // namespace

extern "C" int gstvd_context_append(const gstvd_context_append_t* a, gstvd_stream_t s) {
  if (!a || !a->ctx_ids || !a->ctx_len || !a->new_ids || !a->abnormal || !a->full) return GSTVD_E_NULL;
  if (a->B < 0 || a->T < 1 || a->U < 1 || a->ld_ctx < a->T || a->ld_new < a->U) return GSTVD_E_SHAPE;
  if ((a->segments && a->ld_seg < a->T) || (a->att_mask && a->ld_att < a->T)) return GSTVD_E_SHAPE;
  if (a->B > 0x7fffffff) return GSTVD_E_SHAPE;
  if (a->B == 0) return 0;
  hipLaunchKernelGGL(context_append_kernel, dim3((unsigned)a->B), dim3(WAVE), 0, (hipStream_t)s, *a);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_dialog_rows(const gstvd_dialog_rows_t* a, gstvd_stream_t s) {
  if (!a || !a->cap || !a->ques || !a->ans || !a->ppl || !a->enc_ids || !a->enc_seg || !a->enc_mlm || !a->enc_att || !a->enc_sep ||
      !a->enc_hist_len || !a->dec_ids || !a->dec_labels || !a->dec_att)
    return GSTVD_E_NULL;
  if (a->mask_prob > 0.0 && !a->u_tok) return GSTVD_E_NULL;
  if (a->B < 0 || a->R < 1 || 2 * (int64_t)a->R > a->S || 2 * a->R > WAVE || a->U < 1 || a->U > UMAX || a->Lc < 1 || a->Lc > UMAX ||
      a->T < 2 || a->Ud < 3 || a->n_special < 0 || a->n_special > 8)
    return GSTVD_E_SHAPE;
  if (a->ld_cap < a->Lc || a->ld_utt < a->U || a->ld_enc < a->T || a->ld_sep < a->S || a->ld_dec < a->Ud || (a->u_tok && a->ld_u < a->T))
    return GSTVD_E_SHAPE;
  const int64_t rows = (int64_t)a->B * a->R;
  if (rows > 0x7fffffff) return GSTVD_E_SHAPE;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(dialog_rows_kernel, dim3((unsigned)rows), dim3(WAVE), 0, (hipStream_t)s, *a);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
