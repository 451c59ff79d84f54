"""Scoring given captions against the forward-only calls that existed before it, at the C2 training
shape (B = 64, N = 36 x 2048 features, T = 20, V = 10000; bf16 and fp32, random-init weights, synthetic
batch), in milliseconds per call:

  score          Engine.score_captions(feats, pos, caps)                            R = 64
  loss           Engine.compute_loss(feats, pos, caps) in eval mode                  R = 64
  score_idx      Engine.score_captions(..., img_idx) on 5 x 64 captions of 64 images  R = 320
  weighted_idx   Engine.train_step_weighted(..., img_idx, train=False), same rows    R = 320

Each figure: warm-up calls, then a host clock around --calls (>= 200) calls between two device
synchronisations.  One process measures one library (CAPGEN_LIB_PATH, default the built one; a library
without capgen_score_captions gets the two older calls only) and prints one JSON line.

--parent LIB --rounds K: K alternating rounds, LIB (the parent commit's libcapgen.so) first in each, one
fresh process per measurement; prints the table and the parent's own round-to-round spread, the yardstick
for any difference (--out FILE also writes it there)."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-caption_amd"))
NAMES = ("score", "loss", "score_idx", "weighted_idx")


def timed(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def measure(calls, warmup):
    import torch

    from capgen import _lib, preset
    from capgen.engine import Engine
    from capgen.params import reference_init_state_dict
    from capgen.synthetic import synthetic_batch
    # an older library (the parent's) lacks the scoring symbols: bind what it has, time the older calls
    missing = [s for s in _lib._SIGS if s.startswith(("capgen_score", "capgen_debug_score")) and
               not _symbol(_lib.LIB_PATH, s)]
    for s in missing:
        del _lib._SIGS[s]
    has_score = not missing
    B, N, T, n = 64, 36, 20, 5
    out = {"lib": _lib.LIB_PATH, "calls": calls}
    for dtype in ("bf16", "fp32"):
        cfg = preset("C2", dtype=dtype)
        e = Engine(cfg, "cuda:0")
        e.load_state_dict({k: torch.from_numpy(v) for k, v in reference_init_state_dict(cfg, seed=0).items()})
        e.set_training(False)
        f, p, c = synthetic_batch(B, N, cfg.encode_dim_features, cfg.encode_dim_positions, T, cfg.num_vocab, seed=1000)
        f = f.cuda().bfloat16() if dtype == "bf16" else f.cuda()
        p, c = p.cuda(), c.cuda().to(torch.int32)
        caps5 = torch.cat([c.roll(j, 0) for j in range(n)]).contiguous()
        idx = torch.arange(B, dtype=torch.int32, device="cuda:0").repeat(n)
        w = torch.ones(n * B, device="cuda:0")
        res = {}
        if has_score:
            res["score"] = timed(lambda: e.score_captions(f, p, c), calls, warmup)
        res["loss"] = timed(lambda: e.compute_loss(f, p, c), calls, warmup)
        if has_score:
            res["score_idx"] = timed(lambda: e.score_captions(f, p, caps5, img_idx=idx), calls, warmup)
        res["weighted_idx"] = timed(lambda: e.train_step_weighted(f, p, caps5, w, img_idx=idx, train=False), calls,
                                    warmup)
        if has_score:  # the two read-outs agree: -sum logp / sum length against the loss
            _, logp, length, _ = e.score_captions(f, p, c)
            res["mean_nll"] = -(logp.double().sum() / length.sum()).item()
            res["compute_loss"] = e.compute_loss(f, p, c).item()
        out[dtype] = {k: round(v, 4) for k, v in res.items()}
        e.close()
    print(json.dumps(out))


def _symbol(path, name):
    import ctypes
    return hasattr(ctypes.CDLL(path), name)


def table(parent, rounds, calls, warmup, out_path):
    new = os.path.join(REPO, "image-caption_amd", "capgen", "libcapgen.so")
    runs = {"parent": [], "new": []}
    for _ in range(rounds):
        for who, lib in (("parent", parent), ("new", new)):
            env = dict(os.environ, CAPGEN_LIB_PATH=os.path.abspath(lib))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(calls), "--warmup",
                                str(warmup)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(r.returncode)
            runs[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
    lines = [f"ms per call, {calls} calls per figure after {warmup} warm-up calls, {rounds} alternating rounds "
             f"(parent library first in each); C2 shape B=64 N=36 T=20 V=10000; R=320 rows for the *_idx calls"]
    for dtype in ("bf16", "fp32"):
        lines.append(f"\n{dtype:5s} {'call':14s} " + " ".join(f"{'parent r' + str(i):>10s} {'new r' + str(i):>10s}"
                                                          for i in range(rounds)) + "   spread(parent)")
        for name in NAMES:
            cells, pv = [], []
            for i in range(rounds):
                a, b = runs["parent"][i][dtype].get(name), runs["new"][i][dtype].get(name)
                pv += [a] if a is not None else []
                cells.append(f"{a:10.4f}" if a is not None else f"{'-':>10s}")
                cells.append(f"{b:10.4f}" if b is not None else f"{'-':>10s}")
            spread = f"{max(pv) - min(pv):.4f}" if pv else "-"
            lines.append(f"      {name:14s} " + " ".join(cells) + f"   {spread}")
        last = runs["new"][-1][dtype]
        lines.append(f"      -sum logp / sum length {last.get('mean_nll')}, compute_loss {last.get('compute_loss')}")
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent", help="the parent commit's libcapgen.so: run the alternating rounds")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.parent:
        table(a.parent, a.rounds, a.calls, a.warmup, a.out)
    else:
        measure(a.calls, a.warmup)
