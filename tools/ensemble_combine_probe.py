"""ensemble_combine alone, at beam-5's C4 shape (R = 1280 rows, V = 10000) for K = 2 and 3 members (two kernel
instances, so the profiler's statistics keep them apart), one mode, with or without the slab stats: `--reps`
launches per K through capgen_debug_ensemble_combine, rotating over `--sets` sets of input / output buffers so
that no launch finds its inputs in a cache (a set is (K + 1) x 51 MB).  Meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/ensemble_combine_probe.py`, which gives the kernel's own time;
without the profiler it prints the wall time per launch (launch overhead included).
Bytes moved per launch, the figure to divide by the time: K reads + 1 write of R x V f32 (the second read of each
member row is served by L2), plus R x 625 x 8 for the stats."""
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-caption_amd"))
import torch  # noqa: E402

from capgen import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1280)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--mode", default="prob", choices=("prob", "logprob"))
    ap.add_argument("--no-stats", action="store_true")
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    R, V = args.rows, args.vocab
    g = torch.Generator(device="cpu").manual_seed(1)
    sets = []
    for _ in range(args.sets):
        z = [(3 * torch.randn(R, V, generator=g)).to(dev) for _ in range(3)]
        sets.append((z, torch.empty(R, V, device=dev), torch.empty(R, (V + 15) // 16, 2, device=dev)))
    mode, stats = ("prob", "logprob").index(args.mode), not args.no_stats
    for K in (2, 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.reps):
            z, out, st = sets[i % args.sets]
            ptrs = (C.c_void_p * K)(*[t.data_ptr() for t in z[:K]])
            _lib.check(lib.capgen_debug_ensemble_combine(ptrs, None, K, mode, R, V, C.c_void_p(out.data_ptr()),
                                                         C.c_void_p(st.data_ptr()) if stats else None, None))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.reps
        nbytes = (K + 1) * R * V * 4 + (R * ((V + 15) // 16) * 8 if stats else 0)
        print(json.dumps({"K": K, "mode": args.mode, "stats": stats, "rows": R, "vocab": V,
                          "wall_us_per_launch": round(dt * 1e6, 1), "bytes": nbytes}), flush=True)


if __name__ == "__main__":
    main()
