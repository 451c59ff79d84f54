"""One rank of a data-parallel run with weight decay and the averaged weights on (launched by
tests/test_gpu_optim_world2.py through torch.distributed.run; rank r on GPU r), modelled on
tests/dp_world2_worker.py: rank r trains the fp32 engine on its 1/world slice of the c1 fixture batch,
tries swap_ema() before capgen_dp_sync_adam_state (stale under ZeRO-1 at world > 1), synchronises,
swaps in and out, and writes parameters, average and what the early swap said to <out>.r<rank>.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "image-caption_amd")]

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

WD, D = 0.1, 0.9


def main():
    zero, steps, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    from capgen import _lib
    from capgen.dp import init_engine_dp
    from capgen.engine import Engine
    from capgen.params import fixture_state_dict
    from golden_util import fixture_inputs, load_fixture

    _lib.set_knob("ZERO", zero)
    dev = f"cuda:{rank}"
    cfg, seed, z = load_fixture("c1")
    f, p, c = (t.to(dev) for t in fixture_inputs(z))
    h = c.shape[0] // world
    sl = slice(rank * h, (rank + 1) * h)
    f, p, c = f[sl], p[sl], c[sl]
    e = Engine(cfg.replace(dtype="fp32"), dev)
    e.load_state_dict(fixture_state_dict(cfg, seed=seed, with_buffer=False))
    e.set_training(False)
    init_engine_dp(e, rank, world)
    e.set_weight_decay(WD)
    e.set_ema(D)
    losses = [e.train_step(f, p, c).item() for _ in range(steps)]
    torch.cuda.synchronize()
    early = ""
    try:
        e.swap_ema()
        e.swap_ema()  # (not stale: it went through; back out again)
    except RuntimeError as err:
        early = str(err)
    dist.barrier()
    e.dp_sync_adam_state()
    params, ema = e.params_arena(), e.ema_arena()
    e.swap_ema()
    swapped_ok = np.array_equal(e.params_arena().view(np.int32), ema.view(np.int32))
    e.swap_ema()
    np.savez(f"{out}.r{rank}.npz", params=params, ema=ema, losses=np.array(losses), early=np.array([early]),
             swapped_ok=np.array([swapped_ok]), n_updates=np.array([e.ema_info()[1]]),
             comm=np.array([e.dp_comm_info()[0]]))
    dist.barrier()
    e.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
