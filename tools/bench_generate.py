"""C4 (BASELINE.json configs[3]): generate() on 1 GPU — beam 5 and greedy over a batch of 256
images (36 x 2048 region features, max_length 20), bf16, synthetic inputs, random-init C2
weights.  KV-cached decode (model.py:101-200 restated).  Prints one JSON line per mode.
sample1 / sample5: sampled decoding (Engine.sample, n_samples 1 / 5, top_k 0, temperature 1) -- the
decode steps of greedy (B rows) / beam-5 (5 B rows) with one selection launch per token, so they are
read against those two modes of the same run.  sample1p / sample5p: the same with top_p = 0.9 (nucleus
sampling).  The random-init weights give nearly flat logits, the worst case of the nucleus selection.
beam5e / beam5en: the beam search that stops at <END> (Engine.beam_nbest, beam 5, <END> = id 2) with
length_penalty 0 and n_best 1 / length_penalty 1 and n_best 5 -- beam5's launches plus one finish kernel, read
against beam5 of the same run.
beam5ec / sample1c: beam5e / sample1 under decode constraints (Engine.set_decode_constraints: no_repeat_ngram 2,
min_length 5, repetition_penalty 1.2, three banned words) -- one more launch per decode step, read against
beam5e / sample1 of the same run.
ens2_beam5e / ens3_beam5e / ens2_sample1: beam5e / sample1 over an ensemble of 2 / 3 engines (random-init C2
weights of seeds 0, 1, 2; capgen.engine.ensemble_beam_nbest / ensemble_sample, equal weights, mode 'prob'): every
member's decoder steps plus one ensemble_combine launch per step, read against K x the single-engine mode of the
same run.
beam6 / beam6g3: Engine.beam_nbest at beam 6 and diverse beam search (Engine.beam_diverse, beam 6 in 3 groups,
diversity_penalty 0.5), both with <END> = id 2, length_penalty 0 and n_best 1 (per group): the same decoder steps;
beam6g3 selects with the full-row top-k, the group merge and the three reorder launches per token where bf16
beam6 takes one fused launch, so it is read against beam6 of the same run.  --dtype fp32 runs every mode on the
fp32 engine.
beam5f2: forced-word beam search (Engine.beam_forced) at beam 5 with two single-word groups per image, the words
drawn from a fixed seed (ids 3 .. num_vocab - 1, two distinct per image), <END> = id 2, length_penalty 0, n_best 1:
beam5e's decoder steps; the selection is the full-row top-k with 8 finalists and 2 word scores per row, the bank
merge and the three reorder launches per token where bf16 beam5e takes one fused launch, so it is read against
beam5e of the same run.

Algorithmic work (KV-cached count): beam-5 1776.7 GFLOP, greedy 699.4 GFLOP per
256-image batch.  The reference CPU path (no KV cache) took 25.0 s (beam) / 5.87 s (greedy) per
batch on the survey container's 8 cores."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-caption_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from capgen import _lib, preset  # noqa: E402
from capgen.engine import Engine, ensemble_beam_nbest, ensemble_sample  # noqa: E402
from capgen.params import reference_init_state_dict  # noqa: E402
from capgen.synthetic import synthetic_batch  # noqa: E402

GFLOP = {"beam5": 1776.7, "greedy": 699.4, "sample1": 699.4, "sample5": 1776.7,  # (sampleN: its decode steps')
         "sample1p": 699.4, "sample5p": 1776.7, "beam5e": 1776.7, "beam5en": 1776.7,
         "beam5ec": 1776.7, "sample1c": 699.4,
         "beam6": 2046.0, "beam6g3": 2046.0,  # (beam5 + one more row's decoder steps: (1776.7 - 699.4) / 4)
         "beam5f2": 1776.7,
         "ens2_beam5e": 2 * 1776.7, "ens3_beam5e": 3 * 1776.7, "ens2_sample1": 2 * 699.4}  # (every member's steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1, help="untimed calls first (the first one tunes GEMM shapes and sizes the workspaces)")
    ap.add_argument("--modes", default="beam5,greedy", help="of beam5, greedy, sample1, sample5, sample1p, sample5p, beam5e, beam5en, beam5ec, sample1c, "
                    "ens2_beam5e, ens3_beam5e, ens2_sample1, beam6, beam6g3, beam5f2")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    args = ap.parse_args()
    cfg = preset("C2", dtype=args.dtype)
    dev = torch.device("cuda", 0)
    eng = Engine(cfg, dev)
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in reference_init_state_dict(cfg, seed=0).items()})
    eng.set_training(False)
    members = [eng]  # the ensemble modes' engines: created when the first of them runs

    def ensemble(K):
        while len(members) < K:
            e = Engine(cfg, dev)
            e.load_state_dict({k: torch.from_numpy(v)
                               for k, v in reference_init_state_dict(cfg, seed=len(members)).items()})
            e.set_training(False)
            members.append(e)
        return members[:K]

    B, N = args.batch, 36
    f, p, _ = synthetic_batch(B, N, cfg.encode_dim_features, cfg.encode_dim_positions, cfg.max_length,
                              cfg.num_vocab, seed=7)
    f = f.to(dev, torch.bfloat16 if args.dtype == "bf16" else torch.float32).contiguous()
    p = p.to(dev).contiguous()
    rng = np.random.default_rng(11)  # beam5f2's words: two per image, each its own group
    f2_word = np.stack([rng.choice(np.arange(3, cfg.num_vocab), 2, replace=False) for _ in range(B)]).astype(np.int32)
    f2_group = np.tile(np.arange(2, dtype=np.int32), (B, 1))
    runs = {"beam5": lambda: eng.beam(f, p, 5), "greedy": lambda: eng.greedy(f, p, want_attention=False),
            "sample1": lambda: eng.sample(f, p, n_samples=1, seed=1), "sample5": lambda: eng.sample(f, p, n_samples=5, seed=1),
            "sample1p": lambda: eng.sample(f, p, n_samples=1, seed=1, top_p=0.9),
            "sample5p": lambda: eng.sample(f, p, n_samples=5, seed=1, top_p=0.9),
            "beam5e": lambda: eng.beam_nbest(f, p, 5, 2, length_penalty=0.0, n_best=1),
            "beam5en": lambda: eng.beam_nbest(f, p, 5, 2, length_penalty=1.0, n_best=5),
            "beam5ec": lambda: eng.beam_nbest(f, p, 5, 2, length_penalty=0.0, n_best=1),
            "sample1c": lambda: eng.sample(f, p, n_samples=1, seed=1),
            "beam6": lambda: eng.beam_nbest(f, p, 6, 2, length_penalty=0.0, n_best=1),
            "beam6g3": lambda: eng.beam_diverse(f, p, 6, 3, 0.5, 2, length_penalty=0.0, n_best=1),
            "beam5f2": lambda: eng.beam_forced(f, p, 5, 2, f2_word, f2_group, length_penalty=0.0, n_best=1),
            "ens2_beam5e": lambda: ensemble_beam_nbest(ensemble(2), f, p, 5, 2, length_penalty=0.0, n_best=1),
            "ens3_beam5e": lambda: ensemble_beam_nbest(ensemble(3), f, p, 5, 2, length_penalty=0.0, n_best=1),
            "ens2_sample1": lambda: ensemble_sample(ensemble(2), f, p, n_samples=1, seed=1)}
    for name, fn in runs.items():
        if name not in args.modes.split(","):
            continue
        if name.endswith("c"):
            eng.set_decode_constraints(no_repeat_ngram=2, min_length=5, end_id=2, repetition_penalty=1.2, banned=(0, 1, 3))
        else:
            eng.set_decode_constraints()
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.reps
        print(json.dumps({"metric": f"generate {name} images/sec (C4: B={B}, max_length={cfg.max_length})",
                          "value": round(B / dt, 1), "unit": "images/s", "ms_per_batch": round(dt * 1e3, 3),
                          "achieved_tflops": round(GFLOP[name] * (B / 256) / dt / 1e3, 2), "dtype": args.dtype,
                          "data": "synthetic", "gemm_shapes_tuned_live": _lib.tune_live_count()}), flush=True)


if __name__ == "__main__":
    main()
