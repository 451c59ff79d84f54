"""Cost of weight decay and the averaged weights on the benchmarked step: bench.py's workload and timing
loop (C2, bf16, batch 64, 36 regions, seq_len 20, dropout 0.3; HIP events around --steps steps after
--warmup) with one setting per process, as tools/bench_gradclip.py (several engines in one process do
not compare, see there):

    (no option)        no setter call: the default update, what bench.py times
    --weight-decay W   set_weight_decay(W): one more multiply in the update kernel, one more word in its prep
    --ema-decay D      set_ema(D): the average's arena joins the update's streams (38 B per parameter, not 30)
    --max-norm X       set_grad_clip(X) with them: every bucket's update on the step's tail

With --ema-decay it also times swap_ema() after the loop: the exchange of the two arenas plus the re-cast
of the bf16 shadow and the re-tiling, the one-off cost of evaluating on the average (mean of --swaps calls,
host-synchronous as the call is).  Prints one JSON line.  Compare settings by alternating runs of this
script."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-caption_amd"))

import torch  # noqa: E402

B, N, T = 64, 36, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--weight-decay", type=float, default=None, help="set_weight_decay value (default: off)")
    ap.add_argument("--ema-decay", type=float, default=None, help="set_ema value (default: off)")
    ap.add_argument("--max-norm", type=float, default=None, help="set_grad_clip value (default: clipping off)")
    ap.add_argument("--swaps", type=int, default=4, help="swap_ema() calls to time (an even number)")
    args = ap.parse_args()

    from capgen import _lib, preset
    from capgen.engine import Engine
    from capgen.params import reference_init_state_dict
    from capgen.synthetic import synthetic_batch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = preset("C2", dtype="bf16", dropout=0.3)
    eng = Engine(cfg, dev)
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in reference_init_state_dict(cfg, seed=0).items()})
    if args.max_norm is not None:
        eng.set_grad_clip(args.max_norm)
    if args.weight_decay is not None:
        eng.set_weight_decay(args.weight_decay)
    if args.ema_decay is not None:
        eng.set_ema(args.ema_decay)
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
    swap_ms = None
    if args.ema_decay is not None and args.swaps > 0:
        swaps = args.swaps + args.swaps % 2  # (even: the raw weights are back in place afterwards)
        eng.swap_ema()
        eng.swap_ema()
        t0 = time.perf_counter()
        for _ in range(swaps):
            eng.swap_ema()
        swap_ms = round((time.perf_counter() - t0) * 1e3 / swaps, 4)
    print(json.dumps({"weight_decay": args.weight_decay, "ema_decay": args.ema_decay, "max_norm": args.max_norm,
                      "ms_per_step": round(ev0.elapsed_time(ev1) / args.steps, 4), "steps": args.steps,
                      "warmup": args.warmup, "loss": loss.item(), "arena_elems": eng.arena_elems,
                      "ema_updates": eng.ema_info()[1], "swap_ms": swap_ms}), flush=True)


if __name__ == "__main__":
    main()
