"""The averaged weights under data parallel with several ranks, modelled on tests/test_gpu_dp_world2.py
(needs that many GPUs; the world-1 run of the same launcher and worker runs everywhere): three fp32
steps on the halves of the c1 fixture batch with decay and the average on, ZERO = 1 (the average is
updated in each rank's chunks and all-gathered by capgen_dp_sync_adam_state) and ZERO = 0."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from capgen.params import fixture_state_dict
from golden_util import fixture_inputs, load_fixture
from optim_world2_worker import D, WD

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 3


def _gpus(n):
    return pytest.mark.skipif(torch.cuda.device_count() < n,
                              reason=f"{n} ranks need {n} GPUs (RCCL refuses two ranks on one device)")


def _launch(tmp_path, world, zero, port, timeout=100):
    out = str(tmp_path / f"optim_w{world}_z{zero}")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(HERE, "optim_world2_worker.py"), str(zero), str(STEPS), out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [np.load(f"{out}.r{k}.npz") for k in range(world)]


def _full_batch():
    """one world-1 engine (no communicator) with the same options on the whole fixture batch"""
    from capgen.engine import Engine
    cfg, seed, z = load_fixture("c1")
    f, p, c = (t.to("cuda:0") for t in fixture_inputs(z))
    e = Engine(cfg.replace(dtype="fp32"), "cuda:0")
    e.load_state_dict(fixture_state_dict(cfg, seed=seed, with_buffer=False))
    e.set_training(False)
    e.set_weight_decay(WD)
    e.set_ema(D)
    start = e.ema_arena()
    for _ in range(STEPS):
        e.train_step(f, p, c)
    torch.cuda.synchronize()
    params, ema = e.params_arena(), e.ema_arena()
    e.close()
    assert np.abs(ema - start).max() > 1e-5, "the average did not move: vacuous"
    return params, ema


def test_optim_launcher_world1_fp32(tmp_path):
    (r0,) = _launch(tmp_path, 1, 1, 29640)
    assert int(r0["comm"][0]) == 1 and int(r0["n_updates"][0]) == STEPS
    assert str(r0["early"][0]) == "" and bool(r0["swapped_ok"][0])  # one rank: never stale
    params, ema = _full_batch()
    np.testing.assert_allclose(r0["params"], params, atol=1e-6, rtol=0)
    np.testing.assert_allclose(r0["ema"], ema, atol=1e-6, rtol=0)


@_gpus(2)
@pytest.mark.parametrize("zero,port", [(0, 29641), (1, 29642)])
def test_optim_world2_average_equals_full_batch_fp32(tmp_path, zero, port):
    ranks = _launch(tmp_path, 2, zero, port)
    for z in ranks:
        assert int(z["comm"][0]) == 2 and int(z["n_updates"][0]) == STEPS and bool(z["swapped_ok"][0])
        early = str(z["early"][0])
        if zero:  # sharded: this rank's average was current in its chunks only
            assert "ema_swap" in early and "capgen_dp_sync_adam_state" in early, early
        else:
            assert early == ""
    np.testing.assert_array_equal(ranks[0]["ema"].view(np.int32), ranks[1]["ema"].view(np.int32))
    np.testing.assert_array_equal(ranks[0]["params"].view(np.int32), ranks[1]["params"].view(np.int32))
    params, ema = _full_batch()
    # test_dp_world2_equals_full_batch_fp32's parameter tolerance (summation order of the halves' gradients)
    np.testing.assert_allclose(ranks[0]["params"], params, atol=2e-6, rtol=0)
    np.testing.assert_allclose(ranks[0]["ema"], ema, atol=2e-6, rtol=0)
