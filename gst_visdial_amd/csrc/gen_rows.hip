// Rows of the generative (enc_dec) model on the device: what dataloader/dataloader_visdial_gen.py builds per dialog on the host with a
// tokenizer and Python lists (eval rows :295-458, test rows :507-603, teacher rows :123-293, all through utils/data_utils.py:34-71)
// from token-id pools -- caption, questions, ground-truth answers, the O answer options of every round.  Integer work on token ids,
// ONE launch for a list of encoder rows (dialog, round) and a list of decoder rows (dialog, round, slot), no atomics, workspace or
// host synchronisation.  include/gstvd_hip.h states the rule in full.
//
//   gen_rows_kernel   one wave per output row, the form of disc_rows_kernel (disc_rows.hip); the first n_enc workgroups write the
//                     encoder rows, the next n_dec the decoder rows.  Encoder row: lane g measures context utterance g (caption, q0,
//                     a0, ..: at most 2R <= 64 of them), an inclusive wave scan of len + 1 gives every separator position, each lane
//                     writes its tokens and its [SEP], all lanes zero the tail.  Decoder row: one ballot measures the target, the
//                     lanes write [CLS] x [SEP] 0.. and, in the train modes, the row shifted left.  Every output element is written
//                     once.
#include "common.h"

namespace {

constexpr int UMAX = 64;                                      // tokens of one utterance row (U, Lc <= 64: checked by the host entry)
constexpr int OMAX = 100;                                     // options of a round

DEVFN int utt_len(const int64_t* src, int cap) {              // one lane: the entries in front of the first 0
  int n = 0;
  while (n < cap && src[n] != 0) ++n;
  return n;
}

DEVFN int row_len(const int64_t* src, int cap, int lane) {    // the whole wave, one row of cap <= 64 entries: the same, wave-uniform
  const uint64_t z = __ballot(lane >= cap || src[lane] == 0);
  return z ? __ffsll((long long)z) - 1 : WAVE;
}

DEVFN void enc_row(const gstvd_gen_rows_t& a, int64_t r, int lane) {
  const int T = a.T, U = a.U, R = a.R, S = a.S;
  const int d = a.enc_dialog[r], j = a.enc_round[r];
  int64_t* tok = a.tokens + r * a.ld_row;
  int64_t* seg = a.segments + r * a.ld_row;
  int64_t* mlm = a.mlm + r * a.ld_row;
  float* att = a.att + r * a.ld_row;
  int64_t* sepo = a.sep_indices + r * a.ld_sep;
  if (!(d >= 0 && d < a.D && j >= 0 && j < R)) {              // a row that names nothing: padding, no pool is read
    for (int p = lane; p < T; p += WAVE) { tok[p] = 0; seg[p] = 0; mlm[p] = -1; att[p] = 0.f; }
    for (int s = lane; s < S; s += WAVE) sepo[s] = 0;
    if (lane == 0) a.hist_len[r] = 0;
    return;
  }
  // ---- lane g: context utterance g (caption, q0, a0, ..., qj -- or ..., a(j-1) for the questioner), its length
  const int n_utt = a.mode == GSTVD_GEN_TRAIN_Q ? 2 * j + 1 : 2 * j + 2;
  const int64_t* src = nullptr;
  int len = 0;
  if (lane < n_utt) {
    if (lane == 0) { src = a.cap + (int64_t)d * a.ld_cap; len = utt_len(src, a.Lc); }
    else { src = ((lane & 1) ? a.ques : a.ans) + ((int64_t)d * R + ((lane - 1) >> 1)) * a.ld_utt; len = utt_len(src, U); }
  }
  // ---- inclusive scan of len + 1: the running position of utterance g's [SEP] (position 0 is [CLS])
  const int sep_pos = wave_scan_incl(lane < n_utt ? len + 1 : 0, lane);
  const int total = __shfl(sep_pos, WAVE - 1, WAVE) + 1;      // untruncated row length
  if (lane == 0) {
    tok[0] = a.cls; seg[0] = 1; mlm[0] = -1; att[0] = a.cls != 0 ? 1.f : 0.f;
    a.hist_len[r] = n_utt - 1;
  }
  if (lane < n_utt) {
    const int64_t sg = 1 ^ (lane & 1);
    const float* u = a.u_tok ? a.u_tok + r * a.ld_u : nullptr;
    int p = sep_pos - len;                                    // first token of the utterance
    for (int k = 0; k < len && p < T; ++k, ++p) {
      const int64_t v = src[k];
      const bool masked = u != nullptr && (double)u[p] < a.mask_prob;
      const int64_t id = masked ? a.mask_id : v;
      tok[p] = id; seg[p] = sg; mlm[p] = masked ? v : -1; att[p] = id != 0 ? 1.f : 0.f;
    }
    if (sep_pos < T) { tok[sep_pos] = a.sep; seg[sep_pos] = sg; mlm[sep_pos] = -1; att[sep_pos] = a.sep != 0 ? 1.f : 0.f; }
  }
  for (int p = total + lane; p < T; p += WAVE) { tok[p] = 0; seg[p] = 0; mlm[p] = -1; att[p] = 0.f; }
  for (int s = lane; s < S; s += WAVE) sepo[s] = s < n_utt ? sep_pos : 0;   // s < n_utt <= 64: s is this lane
}

DEVFN void dec_row(const gstvd_gen_rows_t& a, int64_t r, int lane) {
  const int U = a.U, R = a.R, O = a.O, Ud = a.Ud;
  const int d = a.dec_dialog[r], j = a.dec_round[r], slot = a.dec_slot[r];
  const bool train = a.mode == GSTVD_GEN_TRAIN_A || a.mode == GSTVD_GEN_TRAIN_Q;
  int64_t* ids = a.dec_ids + r * a.ld_dec;
  float* att = a.dec_att + r * a.ld_dec;
  int64_t* lab = train ? a.dec_labels + r * a.ld_dec : nullptr;

  bool ok = d >= 0 && d < a.D && j >= 0 && j < R && slot >= 0 && (train ? slot == 0 : slot < a.num_options);
  const int64_t dj = ok ? (int64_t)d * R + j : 0;
  int c = -1;
  const int64_t* x_src = nullptr;
  if (ok) {
    if (train) x_src = (a.mode == GSTVD_GEN_TRAIN_A ? a.ans : a.ques) + dj * a.ld_utt;
    else {
      if (a.mode == GSTVD_GEN_EVAL) {
        const int64_t gt = a.gt_index[dj];
        ok = gt >= 0 && gt < O;
        c = slot == 0 ? (int)gt : (slot - 1 < gt ? slot - 1 : slot);
      } else c = slot;
      if (ok) x_src = a.opts + (((int64_t)d * a.Ro + (a.Ro == 1 ? 0 : j)) * O + c) * a.ld_opt;
    }
  }
  if (!ok) {                                                  // a row that names nothing: padding, no pool is read
    for (int i = lane; i < Ud; i += WAVE) { ids[i] = 0; att[i] = 0.f; if (lab) lab[i] = 0; }
    if (lane == 0) a.dec_option[r] = -1;
    return;
  }
  int n = row_len(x_src, U, lane);
  n = n < Ud - 2 ? n : Ud - 2;
  if (lane == 0) a.dec_option[r] = c;
  for (int i = lane; i < Ud; i += WAVE) {
    // [CLS] x [SEP] 0 ...
    const int64_t cur = i == 0 ? a.cls : i <= n ? x_src[i - 1] : i == n + 1 ? a.sep : 0;
    att[i] = cur != 0 ? 1.f : 0.f;
    if (train) {
      const int i1 = i + 1;
      lab[i] = i1 >= Ud ? 0 : i1 <= n ? x_src[i1 - 1] : i1 == n + 1 ? a.sep : 0;
      ids[i] = cur == a.sep ? 0 : cur;                        // behind the shift: [SEP] -> [PAD]
    } else ids[i] = cur;
  }
}

__global__ __launch_bounds__(WAVE) void gen_rows_kernel(gstvd_gen_rows_t a) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (b < a.n_enc) enc_row(a, b, lane);
  else dec_row(a, b - a.n_enc, lane);
}

}  // namespace

extern "C" int gstvd_gen_rows(const gstvd_gen_rows_t* a, gstvd_stream_t s) {
  if (!a || !a->cap || !a->ques || !a->ans) return GSTVD_E_NULL;
  // nulls are reported in front of shapes, the mode included: a mode that is none counts as "not a train mode" here and is refused below
  const bool train = a->mode == GSTVD_GEN_TRAIN_A || a->mode == GSTVD_GEN_TRAIN_Q;
  if (!train && !a->opts) return GSTVD_E_NULL;
  if (a->mode == GSTVD_GEN_EVAL && !a->gt_index) return GSTVD_E_NULL;
  if (a->n_enc > 0 && (!a->enc_dialog || !a->enc_round || !a->tokens || !a->segments || !a->mlm || !a->att || !a->sep_indices || !a->hist_len))
    return GSTVD_E_NULL;
  if (a->n_dec > 0 && (!a->dec_dialog || !a->dec_round || !a->dec_slot || !a->dec_ids || !a->dec_att || !a->dec_option || (train && !a->dec_labels)))
    return GSTVD_E_NULL;
  if (a->mask_prob > 0.0 && !a->u_tok) return GSTVD_E_NULL;
  if (a->mode < GSTVD_GEN_EVAL || a->mode > GSTVD_GEN_TRAIN_Q || a->n_enc < 0 || a->n_dec < 0 || a->n_enc + a->n_dec > 0x7fffffff ||
      a->D < 1 || a->R < 1 || 2 * (int64_t)a->R > a->S || a->S > WAVE || a->U < 1 || a->U > UMAX || a->Lc < 1 || a->Lc > UMAX || a->T < 2 || a->Ud < 3)
    return GSTVD_E_SHAPE;
  if (!train && (a->O < 2 || a->O > OMAX || a->num_options < 2 || a->num_options > a->O || (a->Ro != a->R && a->Ro != 1)))
    return GSTVD_E_SHAPE;
  if (a->ld_cap < a->Lc || a->ld_utt < a->U || (!train && a->ld_opt < a->U) || (a->u_tok && a->ld_u < a->T)) return GSTVD_E_SHAPE;
  if (a->n_enc > 0 && (a->ld_row < a->T || a->ld_sep < a->S)) return GSTVD_E_SHAPE;
  if (a->n_dec > 0 && a->ld_dec < a->Ud) return GSTVD_E_SHAPE;
  if (a->n_enc + a->n_dec == 0) return 0;
  hipLaunchKernelGGL(gen_rows_kernel, dim3((unsigned)(a->n_enc + a->n_dec)), dim3(WAVE), 0, (hipStream_t)s, *a);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
