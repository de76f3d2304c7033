#!/usr/bin/env python3
"""Sample-and-rank answer decoding at the full model size (bf16, 1 GPU, synthetic inputs): 16 dialog rows x 18 tokens, replayed.
  1. ms per call: (a) `sample()` at 16 rows, (b) `sample_ranked` S = 1, (c) S = 4, (d) S = 8, (e) `sample()` at 64 rows with full
     encoder work (what S = 4 would cost as four times the batch), (f) `beam_search` K = 4 -- medians of single replayed calls;
  2. library calls per token of each (from one eagerly issued call);
  3. (a) against (b) in three alternating runs of one session: what the scored launch costs over the plain one.
Writes profiles/sample_ranked.txt (or the path given as the first argument) and prints one JSON line."""
import json, os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
import bench

dev = torch.device("cuda", 0)
model, params = bench.build_model(dev, "bf16", seed=1)
model.eval()
params["mode"] = "vd_gen_val"
V = model.decoder.config.vocab_size
ROWS, STEPS = 16, 18


def inputs(rows, seed):
    d = bench.synthetic_rows(rows, 256, 37, 25, 2048, V, seed, dev)
    kw = {k: d[k] for k in ("enc_image_features", "enc_image_spatials", "enc_image_mask", "enc_input_ids", "enc_segments",
                            "enc_attention_mask")}
    kw["dec_input_ids"] = torch.full((rows, 1), 101, dtype=torch.long, device=dev)
    return kw


def median_ms(fn, n=9, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [round(x, 3) for x in (statistics.median(ts), min(ts), max(ts))]


samp = dict(temperature=0.7, top_k=7, top_p=0.0, ngram_blocking_size=0)
out = {}
with torch.no_grad():
    kw16, kw64 = inputs(ROWS, 7), inputs(ROWS * 4, 8)
    runs = [("a", "sample()       16 rows", lambda: model(**samp, **kw16)),
            ("b", "sample_ranked  16 rows x S = 1", lambda: model.sample_ranked(num_samples=1, **samp, **kw16)),
            ("c", "sample_ranked  16 rows x S = 4", lambda: model.sample_ranked(num_samples=4, **samp, **kw16)),
            ("d", "sample_ranked  16 rows x S = 8", lambda: model.sample_ranked(num_samples=8, **samp, **kw16)),
            ("e", "sample()       64 rows, full encoder work", lambda: model(**samp, **kw64)),
            ("f", "beam_search    16 rows x K = 4", lambda: model.beam_search(num_beams=4, **kw16))]
    for tag, _, fn in runs:
        model.engine.close()                                  # (one pair of captured graphs alive at a time)
        out[tag + "_ms"] = median_ms(fn)
    model.engine.close()
    params["amd_decode_graph"] = False
    for tag, _, fn in runs:
        fn()
        out[tag + "_lib_calls_per_token"] = round(model.engine.decode_lib_calls_per_token, 2)
    params["amd_decode_graph"] = True
    a, b = runs[0][2], runs[1][2]
    ab = []
    for r in range(3):
        ab.append((median_ms(a), median_ms(b)))
    out["a_vs_b"] = ab

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sample_ranked.txt")
with open(path, "w") as f:
    f.write("tools/bench_sample_ranked.py: sample-and-rank answer decoding, full-size bf16 model, %d dialog rows x %d tokens (MI355X)\n" % (ROWS, STEPS))
    f.write("temperature 0.7, top_k 7; medians of 9 single replayed calls after 3 warm-up calls: [median, min, max] ms\n\n")
    f.write("1. ms per call\n")
    for tag, name, _ in runs:
        f.write("  (%s) %-44s %s\n" % (tag, name, out[tag + "_ms"]))
    f.write("\n2. library calls per token (one eagerly issued call)\n")
    for tag, name, _ in runs:
        f.write("  (%s) %-44s %s\n" % (tag, name, out[tag + "_lib_calls_per_token"]))
    f.write("\n3. (a) against (b), three alternating runs of one session: median ms (a), (b), (b) - (a)\n")
    for (ma, mb) in ab:
        f.write("  %8.3f %8.3f %+8.3f\n" % (ma[0], mb[0], mb[0] - ma[0]))
print(json.dumps(out))
