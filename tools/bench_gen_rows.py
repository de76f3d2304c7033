"""Timing of the pooled generative evaluation on the MI355X: 2 dialogs x 10 rounds x 100 options, T = 256, Ud = 25, 37 regions at
the bert-base configs (config.bert_base_enc_config / bert_base_dec_config), bf16, seeded synthetic weights and pools.

    python tools/bench_gen_rows.py --out profiles/gen_rows.txt [--dialogs 2 --iters 200 --repeats 7]

Figures (medians of individually timed iterations with min .. max; no profiler):
  rows launch   gstvd_gen_rows alone, one device-event pair around every launch: the eval chunk of `rounds_per_call` rounds (that
                many encoder rows and 100 decoder rows each), and the random-token rows of the batch (one encoder and one decoder row
                per option)
  pooled        evaluate.score_batch on the pooled batch (pools on the device, one row launch per chunk); one event pair around every whole
                call, so the time the device waits for the host is inside
  loader        evaluate.score_batch on the same batch in the loader's shape -- int64 [dialogs, 10, 100, 256] ids / segments and the
                fp32 mask on the host, each compared with option 0's copy, option 0 shipped chunk by chunk -- which is the path of
                the parent commit, unchanged here
The scores of the two paths are compared bit for bit on the way.  No figure is a pass / fail condition."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def each(fn, iters):
    """One event pair per call: the list of the calls' device times in ms."""
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stat(xs):
    return "median %.4f ms (min %.4f, max %.4f over %d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dialogs", type=int, default=2)
    ap.add_argument("--rounds-per-call", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gen_rows needs an MI355X: no device, no number")
    import bench
    from gst_visdial_amd import ops, gen_rows, evaluate as EV
    from gst_visdial_amd.config import bert_base_enc_config, bert_base_dec_config
    dev = torch.device("cuda:0")
    model, params = bench.build_model(dev, "bf16", seed=1)
    model.eval()
    D, R, O, U, Lc, T, Ud, regions = a.dialogs, 10, 100, 18, 38, 256, 25, 37
    vocab, feat = bert_base_dec_config()["vocab_size"], bert_base_enc_config()["v_feature_size"]
    params = dict(params, mode="vd_eval_val", max_seq_len=T, max_utt_len=Ud, num_options=O)
    g = torch.Generator().manual_seed(1)

    def utts(*shape):                                                     # 0-padded rows of 1 .. U ordinary ids
        ids = torch.randint(1000, vocab, shape, generator=g)
        lens = torch.randint(1, shape[-1] + 1, shape[:-1], generator=g)
        return ids * (torch.arange(shape[-1]) < lens.unsqueeze(-1))
    gt = torch.randint(0, O, (D, R), generator=g)
    opts = utts(D, R, O, U)
    pools = dict(cap=utts(D, Lc), ques=utts(D, R, U), opts=opts, ans=torch.gather(opts, 2, gt.view(D, R, 1, 1).expand(D, R, 1, U)).squeeze(2),
                 gt_index=gt, enc_image_feat=torch.randn(D, regions, feat, generator=g),
                 enc_image_loc=torch.rand(D, regions, 5, generator=g), enc_image_mask=torch.ones(D, regions))
    pooled = {k: v.to(dev) for k, v in pools.items()}
    n = D * R * O
    # the same batch in the loader's shape, on the host (built here by the kernel, copied back and repeated per option)
    it = gen_rows.eval_rounds(pooled, 0, D * R, params)
    rep = lambda k: it[k].cpu().view(D, R, 1, -1).expand(D, R, O, -1).contiguous()
    loader = dict(enc_input_ids=rep("enc_input_ids"), enc_segments=rep("enc_segments"), enc_att_mask=rep("enc_att_mask"),
                  dec_input_ids=it["dec_input_ids"].cpu().view(D, R, O, Ud), dec_att_mask=it["dec_att_mask"].cpu().view(D, R, O, Ud),
                  **{k: pools[k] for k in gen_rows.IMAGE_KEYS})
    del it
    text_bytes = sum(loader[k].numel() * loader[k].element_size() for k in ("enc_input_ids", "enc_segments", "enc_att_mask", "dec_input_ids", "dec_att_mask"))
    pool_bytes = sum(pools[k].numel() * pools[k].element_size() for k in gen_rows.POOL_KEYS)

    rounds = min(a.rounds_per_call, D * R)
    chunk = lambda: gen_rows.eval_rounds(pooled, 0, rounds, params)
    noisy_params = dict(params, attack="random_token", mask_prob=0.15)
    u_tok = torch.rand(n, T, device=dev)
    noisy = lambda: gen_rows.eval_rounds(pooled, 0, D * R, noisy_params, u_tok)
    # the launch alone: the row lists built once, outside the timed call
    def launch_of(p, u):
        flat = torch.arange(0, (rounds if u is None else D * R) * O, device=dev)
        dd, dj, ds = (flat // (R * O)).to(torch.int32), ((flat // O) % R).to(torch.int32), (flat % O).to(torch.int32)
        if u is None:
            r = torch.arange(rounds, device=dev)
            enc = ((r // R).to(torch.int32), (r % R).to(torch.int32))
        else:
            enc = (dd, dj)
        out = ops.gen_rows(pooled["cap"], pooled["ques"], pooled["ans"], pooled["opts"], pooled["gt_index"], "eval", T, Ud, enc, (dd, dj, ds),
                           num_options=O, mask_prob=p, u_tok=u)
        return lambda: ops.gen_rows(pooled["cap"], pooled["ques"], pooled["ans"], pooled["opts"], pooled["gt_index"], "eval", T, Ud, enc,
                                    (dd, dj, ds), num_options=O, mask_prob=p, u_tok=u, out=out)
    k_chunk, k_noisy = launch_of(0.0, None), launch_of(0.15, u_tok)
    for f in (chunk, noisy, k_chunk, k_noisy):
        f()
    torch.cuda.synchronize()
    chunk_ms, noisy_ms = each(k_chunk, a.iters), each(k_noisy, a.iters)
    item_ms, nitem_ms = each(chunk, a.iters), each(noisy, a.iters)

    score_p = lambda: EV.score_batch(model, pooled, dev, a.rounds_per_call, params=params)
    score_l = lambda: EV.score_batch(model, loader, dev, a.rounds_per_call)
    _, sp = wall(score_p)                                                 # warm-up of both: arena, every shape
    _, sl = wall(score_l)
    same = torch.equal(sp.float().view(torch.int32), sl.float().view(torch.int32))
    p_ms, l_ms = [], []
    for _ in range(a.repeats):                                            # alternating, so a drift of the machine meets both
        p_ms += each(score_p, 1)
        l_ms += each(score_l, 1)
    lines = [
        "generative rows from pools: %d dialogs x %d rounds x %d options = %d option rows, T = %d, Ud = %d, %d regions, bert-base configs, bf16, MI355X"
        % (D, R, O, n, T, Ud, regions),
        "gstvd_gen_rows alone, eval chunk: %d encoder + %d decoder rows (one event pair per launch):      %s" % (rounds, rounds * O, stat(chunk_ms)),
        "gstvd_gen_rows alone, random-token rows: %d encoder + %d decoder rows, mask_prob 0.15:          %s" % (n, n, stat(noisy_ms)),
        "gen_rows.eval_rounds, the same chunk with its index arithmetic and allocations:                  %s" % stat(item_ms),
        "gen_rows.eval_rounds, the random-token rows likewise:                                            %s" % stat(nitem_ms),
        "score_batch, pooled batch (%d chunk(s) of %d rounds; one event pair per call):                    %s" % (-(-D * R // a.rounds_per_call), a.rounds_per_call, stat(p_ms)),
        "score_batch, loader-shaped batch on the host (the parent commit's path: 3 comparisons, copies):  %s" % stat(l_ms),
        "pooled / loader (medians): %.4f" % (statistics.median(p_ms) / statistics.median(l_ms)),
        "text bytes of the loader-shaped batch: %d (%.1f MB), of which the scorer ships option 0's copy; the pools: %d bytes (%.2f MB), resident"
        % (text_bytes, text_bytes / 1e6, pool_bytes, pool_bytes / 1e6),
        "scores of the two paths bit-equal: %s" % same,
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
