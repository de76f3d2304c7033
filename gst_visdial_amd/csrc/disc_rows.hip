// Rows of the discriminative (enc_only) model on the device: what dataloader/dataloader_visdial_disc.py builds per dialog on the
// host with a tokenizer and Python lists (train rows :125-288, eval rows :299-401, both through utils/data_utils.py:34-71) from
// token-id pools -- caption, questions, ground-truth answers, the O answer options of every round.  Integer work on token ids, ONE
// launch for any list of (dialog, round, slot) rows, no atomics, workspace or host synchronisation.  include/gstvd_hip.h states the
// rule in full.
//
//   disc_rows_kernel   one wave per output row (d, j, slot), the form of dialog_rows_kernel (dialog.hip).  Lane g measures context
//                      utterance g (caption, q0, a0, .., qj: 2j + 2 <= 64 of them).  A train-mode negative is chosen first: the
//                      lanes measure the <= 100 options in two passes of 64, two ballots each give the candidate and the feasible
//                      sets, and the draw picks the k-th set bit.  Then pruneRounds shifts the lanes (lane i owns utterance
//                      i + drop), an inclusive wave scan of len + 1 gives every separator position, each lane writes its tokens and
//                      its [SEP], all lanes zero the tail.  Every output element is written once.
#include "common.h"

namespace {

constexpr int UMAX = 64;                                      // tokens of one utterance row (U, Lc <= 64: checked by the host entry)
constexpr int OMAX = 100;                                     // options of a round: two ballots cover them

DEVFN int utt_len(const int64_t* src, int cap) {              // one lane: the entries in front of the first 0
  int n = 0;
  while (n < cap && src[n] != 0) ++n;
  return n;
}

DEVFN int row_len(const int64_t* src, int cap, int lane) {    // the whole wave, one row of cap <= 64 entries: the same, wave-uniform
  const uint64_t z = __ballot(lane >= cap || src[lane] == 0);
  return z ? __ffsll((long long)z) - 1 : WAVE;
}

DEVFN int kth_set(uint64_t lo, uint64_t hi, int k) {          // index of the k-th set bit of the 128-bit set (k < its popcount)
  const int nlo = __popcll(lo);
  uint64_t m = k < nlo ? lo : hi;
  for (int i = k < nlo ? k : k - nlo; i > 0; --i) m &= m - 1;
  return (k < nlo ? 0 : 64) + __ffsll((long long)m) - 1;
}

DEVFN int pick(float u, int n) {                              // min(floor((double)u * n), n - 1); u * n is exact in double
  const double x = floor((double)u * (double)n);
  return x >= (double)n ? n - 1 : x > 0.0 ? (int)x : 0;
}

__global__ __launch_bounds__(WAVE) void disc_rows_kernel(gstvd_disc_rows_t a) {
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int T = a.T, U = a.U, R = a.R, O = a.O, S = a.S;
  const int d = a.row_dialog[r], j = a.row_round[r], slot = a.row_slot[r];
  int64_t* tok = a.tokens + r * a.ld_row;
  int64_t* seg = a.segments + r * a.ld_row;
  int64_t* mlm = a.mask + r * a.ld_row;
  float* att = a.att + r * a.ld_row;
  int64_t* sepo = a.sep_indices + r * a.ld_sep;

  bool ok = d >= 0 && d < a.D && j >= 0 && j < R && slot >= 0 && (a.train || slot < a.num_options);
  const int64_t dj = ok ? (int64_t)d * R + j : 0;
  const int64_t gt64 = ok ? a.gt_index[dj] : -1;
  ok = ok && gt64 >= 0 && gt64 < O;
  if (!ok) {                                                  // a row that names nothing: padding, no pool is read
    for (int p = lane; p < T; p += WAVE) { tok[p] = 0; seg[p] = 0; mlm[p] = -1; att[p] = 0.f; }
    for (int s = lane; s < S; s += WAVE) sepo[s] = 0;
    if (lane == 0) {
      a.hist_len[r] = 0;
      if (a.neg_option) a.neg_option[r] = -1;
      if (a.train) { a.nsp_labels[2 * r] = 0.f; a.nsp_labels[2 * r + 1] = 0.f; }
    }
    return;
  }
  const int gt = (int)gt64;

  // ---- lane g: context utterance g (caption, q0, a0, ..., qj), its length
  const int n_ctx = 2 * j + 2;
  int len = 0;
  if (lane < n_ctx) {
    if (lane == 0) len = utt_len(a.cap + (int64_t)d * a.ld_cap, a.Lc);
    else len = utt_len(((lane & 1) ? a.ques : a.ans) + ((int64_t)d * R + ((lane - 1) >> 1)) * a.ld_utt, U);
  }

  // ---- the last utterance x (wave-uniform): its source row, its length, the option it is
  const int64_t* x_src;
  int x_len, c = -1;
  float lab0 = 1.f, lab1 = 0.f;
  if (!a.train) {
    c = slot == 0 ? gt : (slot - 1 < gt ? slot - 1 : slot);
    x_src = a.opts + (dj * O + c) * a.ld_opt;
    x_len = row_len(x_src, U, lane);
  } else if (slot == 0) {
    x_src = a.ans + dj * a.ld_utt;
    x_len = row_len(x_src, U, lane);
  } else {
    const int len_a = row_len(a.ans + dj * a.ld_utt, U, lane);
    int ctx = lane < n_ctx ? len + 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ctx += __shfl_xor(ctx, o, WAVE);
    const int tot_len = 1 + ctx + len_a + 1;                  // the loader's running length: a_j counted
    uint64_t cand[2], feas[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int o = lane + h * WAVE;
      const bool is_c = o < O && o != gt && o - (o > gt ? 1 : 0) < a.num_options - 1;
      const int l = is_c ? utt_len(a.opts + (dj * O + o) * a.ld_opt, U) : 0;
      cand[h] = __ballot(is_c);
      feas[h] = __ballot(is_c && T >= tot_len + l + 1);
    }
    const int n_f = __popcll(feas[0]) + __popcll(feas[1]), n_c = __popcll(cand[0]) + __popcll(cand[1]);
    const float u = a.u_neg[r];
    c = n_f > 0 ? kth_set(feas[0], feas[1], pick(u, n_f)) : kth_set(cand[0], cand[1], pick(u, n_c));
    x_src = a.opts + (dj * O + c) * a.ld_opt;
    x_len = row_len(x_src, U, lane);
    if (n_f == 0 && len_a < x_len) x_len = len_a;             // nothing fits: the loader cuts the option to the answer's length
    lab0 = 0.f; lab1 = 1.f;
    if (a.dense_scores) {
      const double s = a.dense_scores[dj * O + c];
      lab0 = (float)s; lab1 = (float)(1.0 - s);
    }
  }

  // ---- pruneRounds: lane i owns utterance i + drop of the 2j + 3
  const int n_all = n_ctx + 1;
  const int drop = j + 2 > a.tot_rounds ? n_all - 2 * a.tot_rounds : 0;
  const int n_utt = n_all - drop;
  const int64_t start_seg = drop ? 0 : 1;
  const int g = lane + drop;
  int my_len = __shfl(len, g & (WAVE - 1), WAVE);
  const int64_t* src = nullptr;
  if (lane < n_utt) {
    if (g == n_ctx) { src = x_src; my_len = x_len; }
    else if (g == 0) src = a.cap + (int64_t)d * a.ld_cap;
    else src = ((g & 1) ? a.ques : a.ans) + ((int64_t)d * R + ((g - 1) >> 1)) * a.ld_utt;
  }
  // ---- inclusive scan of len + 1: the running position of utterance i's [SEP] (position 0 is [CLS])
  const int sep_pos = wave_scan_incl(lane < n_utt ? my_len + 1 : 0, lane);
  const int total = __shfl(sep_pos, WAVE - 1, WAVE) + 1;      // untruncated row length = sep_indices[hist_len] + 1
  if (lane == 0) {
    tok[0] = a.cls; seg[0] = start_seg; mlm[0] = -1; att[0] = 1.f;
    a.hist_len[r] = n_utt - 1;
    if (a.neg_option) a.neg_option[r] = c;
    if (a.train) { a.nsp_labels[2 * r] = lab0; a.nsp_labels[2 * r + 1] = lab1; }
  }
  if (lane < n_utt) {
    const int64_t sg = start_seg ^ (lane & 1);
    const float* u = a.u_tok ? a.u_tok + r * a.ld_u : nullptr;
    int p = sep_pos - my_len;                                 // first token of the utterance
    for (int k = 0; k < my_len && p < T; ++k, ++p) {
      const int64_t v = src[k];
      const bool masked = u != nullptr && (double)u[p] < a.mask_prob;
      tok[p] = masked ? a.mask_id : v; seg[p] = sg; mlm[p] = masked ? v : -1; att[p] = 1.f;
    }
    if (sep_pos < T) { tok[sep_pos] = a.sep; seg[sep_pos] = sg; mlm[sep_pos] = -1; att[sep_pos] = 1.f; }
  }
  for (int p = total + lane; p < T; p += WAVE) { tok[p] = 0; seg[p] = 0; mlm[p] = -1; att[p] = 0.f; }
  for (int s = lane; s < S; s += WAVE) sepo[s] = s < n_utt ? sep_pos : 0;   // s < n_utt <= 64: s is this lane
}

}  // namespace

extern "C" int gstvd_disc_rows(const gstvd_disc_rows_t* a, gstvd_stream_t s) {
  if (!a || !a->cap || !a->ques || !a->ans || !a->opts || !a->gt_index || !a->row_dialog || !a->row_round || !a->row_slot ||
      !a->tokens || !a->segments || !a->mask || !a->att || !a->sep_indices || !a->hist_len)
    return GSTVD_E_NULL;
  if (a->mask_prob > 0.0 && !a->u_tok) return GSTVD_E_NULL;
  if (a->train && (!a->u_neg || !a->nsp_labels)) return GSTVD_E_NULL;
  if (a->N < 0 || a->N > 0x7fffffff || a->D < 1 || a->R < 1 || 2 * (int64_t)a->R + 1 > a->S || a->S > WAVE || a->U < 1 || a->U > UMAX ||
      a->Lc < 1 || a->Lc > UMAX || a->O < 2 || a->O > OMAX || a->num_options < 2 || a->num_options > a->O || a->tot_rounds < 1 || a->T < 2)
    return GSTVD_E_SHAPE;
  if (a->ld_cap < a->Lc || a->ld_utt < a->U || a->ld_opt < a->U || a->ld_row < a->T || a->ld_sep < a->S || (a->u_tok && a->ld_u < a->T))
    return GSTVD_E_SHAPE;
  if (a->N == 0) return 0;
  hipLaunchKernelGGL(disc_rows_kernel, dim3((unsigned)a->N), dim3(WAVE), 0, (hipStream_t)s, *a);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
