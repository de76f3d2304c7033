#!/usr/bin/env python3
"""The self-training loop on the device at the full model size (bf16, 1 GPU, random weights, synthetic images): 16 images, ten
rounds, T = 256.  Three alternating runs in one session, medians of 9 calls each ([median, min, max] ms):
  (a) ten `generate.dialog_round` calls (host-side context splice, two host synchronisations per splice);
  (b) `selftrain.generate_dialogs` (the splice in one launch, one flag read behind the loop);
  (c) `selftrain.dialog_train_batch` on (b)'s result (one gstvd_dialog_rows launch + the image noise);
  (d) one student step on that batch: `step.forward` (row candidates and torch.multinomial on the device), backward, FusedAdamW
      -- issued eagerly, without the captured-graph replay and the backward pipeline that bench.py times.
With random weights no [SEP] is ever likely, so every utterance runs to max_seq_len; it is set to 10 here so that ten rounds
(<= 200 tokens) fit behind a caption in T = 256 -- at 18 the contexts of untrained models overflow and then fill up, which both
(a) and (b) report as an error, as the reference does.
Writes profiles/selftrain.txt (or the path given as the first argument) and prints one JSON line."""
import json, os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
import bench
from gst_visdial_amd import step
from gst_visdial_amd.generate import dialog_round
from gst_visdial_amd.optim import FusedAdamW
from gst_visdial_amd.selftrain import generate_dialogs, dialog_train_batch

dev = torch.device("cuda", 0)
IMAGES, ROUNDS, T, MAXLEN, REGIONS = 16, 10, 256, 10, 37
gen_model, gen_params = bench.build_model(dev, "bf16", seed=1)
gen_model.eval()
gen_params["mode"] = "cc12m_gen"
student, st_params = bench.build_model(dev, "bf16", seed=2)
student.train()
opt = FusedAdamW(student, lr=2e-5, warmup_steps=1500, t_total=100000)
V = gen_model.decoder.config.vocab_size

g = torch.Generator().manual_seed(11)
cap = torch.zeros(IMAGES, 38, dtype=torch.long)
for b in range(IMAGES):
    n = int(torch.randint(8, 39, (1,), generator=g))
    cap[b, :n] = torch.randint(1000, min(30000, V), (n,), generator=g)
ids0 = torch.zeros(IMAGES, T, dtype=torch.long)
ids0[:, 0] = 101
ids0[:, 1:39] = cap
ids0[torch.arange(IMAGES), (cap != 0).sum(-1) + 1] = 102
rows = bench.synthetic_rows(IMAGES, T, REGIONS, 25, 2048, V, 7, dev)
base = dict(enc_image_features=rows["enc_image_features"], enc_image_spatials=rows["enc_image_spatials"],
            enc_image_mask=rows["enc_image_mask"], enc_input_ids=ids0.to(dev), enc_segments=(ids0 != 0).long().to(dev),
            enc_input_len=(ids0 != 0).sum(-1).to(dev), dec_input_ids=torch.full((IMAGES, 1), 101, dtype=torch.long, device=dev),
            dec_attention_mask=torch.ones(IMAGES, 1, device=dev))
cap = cap.to(dev)
QK = dict(temperature=0.7, top_k=7, top_p=0.0, ngram_blocking_size=4, max_seq_len=MAXLEN)
AK = dict(temperature=0.7, top_k=7, top_p=0.0, ngram_blocking_size=0, max_seq_len=MAXLEN)
TP = dict(select_data=1, threshold=0.0, mask_prob=0.15, max_seq_len=T, max_utt_len=25)


def fresh():
    return {k: (v.clone() if k.startswith("enc_input") or k == "enc_segments" else v) for k, v in base.items()}


def ten_rounds():
    state = fresh()
    for _ in range(ROUNDS):
        dialog_round(gen_model, gen_model, state, q_kwargs=QK, a_kwargs=AK)
    return state


def whole_dialogs():
    return generate_dialogs(gen_model, gen_model, fresh(), num_rounds=ROUNDS, q_kwargs=QK, a_kwargs=AK)


def student_step(batch):
    loss, _ = step.forward(student, batch, st_params)
    loss.backward()
    opt.step()
    opt.zero_grad()
    return loss


def median_ms(fn, n=9, warm=2):
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


dialogs = whole_dialogs()
TP["threshold"] = float(dialogs["ppl"].median())
batch = dialog_train_batch(dialogs, cap, base, TP)
out = dict(images=IMAGES, rounds=ROUNDS, T=T, max_seq_len=MAXLEN, abnormal_rows=int(dialogs["abnormal"].sum()),
           zeroed_label_rows=int((batch["dec_labels"].reshape(IMAGES * ROUNDS, -1).sum(-1) == 0).sum()),
           context_len_max=int(dialogs["enc_input_len"].max()), runs=[])
for r in range(3):
    out["runs"].append(dict(a=median_ms(ten_rounds), b=median_ms(whole_dialogs),
                            c=median_ms(lambda: dialog_train_batch(dialogs, cap, base, TP)), d=median_ms(lambda: student_step(batch))))
loss = float(student_step(batch).detach())
out["student_loss_finite"] = loss == loss and abs(loss) != float("inf")
med = lambda k: statistics.median(run[k][0] for run in out["runs"])
out["dialogs_per_s"] = round(IMAGES / (med("b") * 1e-3), 2)
out["dialogs_per_s_round_calls"] = round(IMAGES / (med("a") * 1e-3), 2)

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "selftrain.txt")
with open(path, "w") as f:
    f.write("tools/bench_selftrain.py: self-training loop on the device, full-size bf16 models, random weights (MI355X)\n")
    f.write("%d images x %d rounds, T = %d, utterances of max_seq_len = %d tokens, temperature 0.7, top_k 7; decode graphs on\n"
            % (IMAGES, ROUNDS, T, MAXLEN))
    f.write("three alternating runs of one session, medians of 9 calls after 2 warm-up calls: [median, min, max] ms\n\n")
    names = (("a", "ten dialog_round calls"), ("b", "generate_dialogs"), ("c", "dialog_train_batch"),
             ("d", "student step (eager: forward, backward, AdamW)"))
    for r, run in enumerate(out["runs"]):
        for k, name in names:
            f.write("  run %d (%s) %-48s %s\n" % (r + 1, k, name, run[k]))
    f.write("\n  dialogs/s: generate_dialogs %.2f, ten dialog_round calls %.2f (median of the three runs' medians)\n"
            % (out["dialogs_per_s"], out["dialogs_per_s_round_calls"]))
    f.write("  longest final context %d of %d tokens, abnormal rows %d, label rows zeroed by select_data %d of %d, student loss finite: %s\n"
            % (out["context_len_max"], T, out["abnormal_rows"], out["zeroed_label_rows"], IMAGES * ROUNDS, out["student_loss_finite"]))
print(json.dumps(out))
