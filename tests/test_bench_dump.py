"""CPU: bench.py's --dump-outputs writer and its option parsing (no engine, no GPU)."""
import os
import subprocess
import sys
import zlib
from collections import OrderedDict

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeEngine:
    """state_dict() like capgen.engine.Engine: reference-named f32 CPU tensors."""

    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.sd = OrderedDict([
            ("encoder.norm.bias", torch.randn(512, generator=g)),
            ("classifer.weight", torch.randn(700, 512, generator=g)),       # 358400 > DUMP_SAMPLE
            ("small.weight", torch.randn(128, 512, generator=g)),           # 65536 == DUMP_SAMPLE: whole
        ])

    def state_dict(self, with_buffer=True):
        assert with_buffer is False
        return self.sd


def test_dump_outputs_writes_float32_fixed_samples(tmp_path):
    import bench
    a, b = tmp_path / "a", tmp_path / "b"
    eng = _FakeEngine(0)
    bench.dump_outputs(eng, torch.tensor([3.25]), str(a))
    bench.dump_outputs(eng, torch.tensor([3.25]), str(b))
    names = sorted(os.listdir(a))
    assert names == sorted(["loss.npy"] + [f"param.{k}.npy" for k in eng.sd]) == sorted(os.listdir(b))
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(a / "loss.npy").tolist() == [3.25]
    np.testing.assert_array_equal(np.load(a / "param.encoder.norm.bias.npy"), eng.sd["encoder.norm.bias"].numpy())
    np.testing.assert_array_equal(np.load(a / "param.small.weight.npy"), eng.sd["small.weight"].numpy().reshape(-1))
    s = np.load(a / "param.classifer.weight.npy")
    full = eng.sd["classifer.weight"].numpy().reshape(-1)
    assert s.shape == (bench.DUMP_SAMPLE,)
    # the documented recipe: sorted indices without replacement, generator seeded with CRC-32(name)
    idx = np.sort(np.random.default_rng(zlib.crc32(b"classifer.weight")).choice(full.size, size=s.size, replace=False))
    assert np.unique(idx).size == s.size
    np.testing.assert_array_equal(s, full[idx])
    # other values under the same name are sampled at the same places
    other = _FakeEngine(1)
    bench.dump_outputs(other, torch.tensor([0.0]), str(b))
    np.testing.assert_array_equal(np.load(b / "param.classifer.weight.npy"),
                                  other.sd["classifer.weight"].numpy().reshape(-1)[idx])


def test_bench_options_present():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in out.stdout, opt
