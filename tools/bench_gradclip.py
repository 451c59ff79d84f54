"""Cost of gradient clipping on the benchmarked step: bench.py's workload and timing loop (C2, bf16,
batch 64, 36 regions, seq_len 20, dropout 0.3; HIP events around --steps steps after --warmup) with one
clip setting per process, as bench.py has one engine per process:

    (no option)        no setter call: the default schedule, what bench.py times
    --max-norm X       set_grad_clip(X): norm pass per bucket, every bucket's Adam on the step's tail
    --adam-grid G      with it: CAPGEN_CLIP_ADAM_GRID = G workgroups for the deferred Adam (0 = each
                       bucket's own cap, one workgroup per CU) instead of the default

Prints one JSON line.  Compare settings by alternating runs of this script.  (Several engines in one
process do not compare: the second engine created measured 0.6 ms per step slower than the first and
the third at the same setting, whatever the setting -- probably where its three streams land on the
process's few hardware queues; not investigated.)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-caption_amd"))

import torch  # noqa: E402

B, N, T = 64, 36, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max-norm", type=float, default=None, help="set_grad_clip value (default: clipping off)")
    ap.add_argument("--adam-grid", type=int, default=None, help="CAPGEN_CLIP_ADAM_GRID for this run")
    args = ap.parse_args()

    from capgen import _lib, preset
    from capgen.engine import Engine
    from capgen.params import reference_init_state_dict
    from capgen.synthetic import synthetic_batch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = preset("C2", dtype="bf16", dropout=0.3)
    if args.adam_grid is not None:  # (read when the engine is created)
        _lib.set_knob("CLIP_ADAM_GRID", args.adam_grid)
    eng = Engine(cfg, dev)
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in reference_init_state_dict(cfg, seed=0).items()})
    if args.max_norm is not None:
        eng.set_grad_clip(args.max_norm)
    f, p, c = synthetic_batch(B, N, cfg.encode_dim_features, cfg.encode_dim_positions, T, cfg.num_vocab, seed=1000)
    f, p, c = f.to(dev, torch.bfloat16).contiguous(), p.to(dev).contiguous(), c.to(dev).contiguous()
    loss = torch.zeros(1, device=dev)

    for _ in range(args.warmup):
        eng.train_step_raw(f, _lib.BF16, p, c, B, N, T, loss)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(stream)
    for _ in range(args.steps):
        eng.train_step_raw(f, _lib.BF16, p, c, B, N, T, loss)
    ev1.record(stream)
    torch.cuda.synchronize()
    print(json.dumps({"max_norm": args.max_norm, "adam_grid": args.adam_grid,
                      "ms_per_step": round(ev0.elapsed_time(ev1) / args.steps, 4), "steps": args.steps,
                      "warmup": args.warmup, "loss": loss.item(),
                      "grad_norm": eng.grad_norm() if args.max_norm is not None else None}), flush=True)


if __name__ == "__main__":
    main()
