#!/usr/bin/env python3
"""Beam-search answer decoding at the full model size (bf16, 1 GPU, synthetic inputs): 16 dialog rows x 5 beams x 18 tokens.
  * replayed ms per `beam_search` call (encoder graph + the one graph of the whole beam loop), medians of single calls;
  * the share of the beam-step and cache-reorder launches: HIP events around every library call of an EAGER call
    (`ops.Profiler`; events cannot time a kernel inside a replayed graph), reported against that eager call's event total;
  * in the same session `sample()` at 16 rows and at 80 rows (the decoder work of 16 x 5 beams), replayed -- comparisons only;
  * library calls per token of the beam loop.
Writes profiles/beam.txt (or the path given as the first argument) and prints one JSON line."""
import json, os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
import bench
from gst_visdial_amd import ops

dev = torch.device("cuda", 0)
model, params = bench.build_model(dev, "bf16", seed=1)
model.eval()
params["mode"] = "vd_gen_val"
V = model.decoder.config.vocab_size
ROWS, K, STEPS = 16, 5, 18


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
    return statistics.median(ts), min(ts), max(ts)


out = {}
with torch.no_grad():
    kw16, kw80 = inputs(ROWS, 7), inputs(ROWS * K, 8)
    beam = lambda: model.beam_search(num_beams=K, **kw16)
    out["beam_16x5x18_replayed_ms"] = [round(x, 3) for x in median_ms(beam)]
    samp = dict(temperature=0.7, top_k=7, top_p=0.0, ngram_blocking_size=0)
    out["sample_16rows_replayed_ms"] = [round(x, 3) for x in median_ms(lambda: model(**samp, **kw16))]
    out["sample_80rows_replayed_ms"] = [round(x, 3) for x in median_ms(lambda: model(**samp, **kw80))]
    # event-timed shares, eager issue
    params["amd_decode_graph"] = False
    beam()
    out["lib_calls_per_token"] = round(model.engine.decode_lib_calls_per_token, 2)
    with ops.Profiler() as prof:
        beam()
    agg = prof.summary()
    total = sum(a["ms"] for a in agg.values())
    for tag in ("beam_step", "beam_reorder"):
        a = agg.get(tag, dict(ms=0.0, launches=0))
        out[tag] = dict(calls=a["launches"], event_ms=round(a["ms"], 3), us_per_call=round(1e3 * a["ms"] / max(a["launches"], 1), 2),
                        share_of_event_timed_calls=round(a["ms"] / total, 4) if total else None)
    out["event_timed_calls_total_ms"] = round(total, 3)
    params["amd_decode_graph"] = True

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "beam.txt")
with open(path, "w") as f:
    f.write("tools/bench_beam.py: beam-search answer decoding, full-size bf16 model, %d rows x %d beams x %d tokens (MI355X)\n" % (ROWS, K, STEPS))
    f.write("medians of 9 single replayed calls after 3 warm-up calls: [median, min, max] ms\n\n")
    f.write("beam_search 16 x 5, replayed      %s ms per call\n" % out["beam_16x5x18_replayed_ms"])
    f.write("sample()    16 rows, replayed      %s ms per call   (comparison)\n" % out["sample_16rows_replayed_ms"])
    f.write("sample()    80 rows, replayed      %s ms per call   (comparison: the same decoder rows)\n" % out["sample_80rows_replayed_ms"])
    f.write("library calls per token, beam loop  %s\n\n" % out["lib_calls_per_token"])
    f.write("event-timed launches of one eagerly issued call (every library call between two HIP events; total %s ms):\n" % out["event_timed_calls_total_ms"])
    for tag in ("beam_step", "beam_reorder"):
        f.write("  %-13s %s\n" % (tag, json.dumps(out[tag])))
print(json.dumps(out))
