"""C5-style SCST train step on 1 GPU (BASELINE.json configs[4] runs it on 8): B=64 images,
36 x 2048 regions, T=20, the C2 model, bf16; one step = rl_sample (GPU) -> host CIDEr-D +
BLEU-4 scoring (capgen/scst.py) -> rl_finish (GPU: loss, backward, Adam).  Synthetic
vocabulary "w<i>" (V=10000) and random-init weights.  Prints one JSON line with the step
time split into GPU-sample, host-scoring and GPU-finish parts.

--rollouts: the roll-out self-critical step (capgen.models.RolloutSelfCritic) at the same shape:
n_samples = 5 free-running samples per image, greedy baseline, CIDEr-D reward, one weighted
teacher-forced step on the 5 x 64 sampled captions (capgen_train_step_weighted; the caption rows
share the 64 images through img_idx).  Time split into sample, greedy, host reward and weighted step;
also prints capgen_tune_live_count() (0 when the persisted autotune table holds every shape)."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-caption_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from capgen import preset  # noqa: E402
from capgen import _lib  # noqa: E402
from capgen.models import RolloutSelfCritic, SelfCriticNetwork  # noqa: E402
from capgen.params import reference_init_state_dict  # noqa: E402
from capgen.synthetic import synthetic_batch  # noqa: E402


def main(steps=20, warmup=3):
    cfg = preset("C2", dtype="bf16", dropout=0.3)
    vocab = {"<NULL>": 0, "<START>": 1, "<END>": 2}
    vocab.update({f"w{i}": i for i in range(3, cfg.num_vocab)})
    sd = {k: torch.from_numpy(v) for k, v in reference_init_state_dict(cfg, seed=0).items()}
    m = SelfCriticNetwork(config=cfg, word_to_idx=vocab, device="cuda:0", state_dict=sd)
    B, N, T = 64, 36, 20
    f, p, c = synthetic_batch(B, N, cfg.encode_dim_features, cfg.encode_dim_positions, T, cfg.num_vocab, seed=1000)
    f = f.cuda().bfloat16()
    p, c = p.cuda(), c.cuda()
    eng = m.model.engine
    t_s = t_h = t_f = 0.0
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seq, ent, _ = eng.rl_sample(f, p, c)
        seq_h, ent_h = seq.cpu().numpy(), ent.cpu().numpy()
        t1 = time.perf_counter()
        reward = np.broadcast_to(m.scorer.scores(c[:, 1:].cpu().numpy(), seq_h), (B,))
        total = m.scorer.total(reward, ent_h)
        t2 = time.perf_counter()
        out = eng.rl_finish(total, m.structure_loss_weight, train=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if i >= warmup:
            t_s, t_h, t_f = t_s + t1 - t0, t_h + t2 - t1, t_f + t3 - t2
    ms = 1e3 * (t_s + t_h + t_f) / steps
    print(json.dumps({"metric": "SCST train images/sec (C5 step on 1 GPU: B=64, 36x2048 feats, T=20)",
                      "value": round(B / (ms / 1e3), 1), "unit": "images/s", "ms_per_step": round(ms, 3),
                      "split_ms": {"gpu_sample": round(1e3 * t_s / steps, 3), "host_reward": round(1e3 * t_h / steps, 3),
                                   "gpu_finish": round(1e3 * t_f / steps, 3)},
                      "final_loss": round(float(out[0].item()), 4), "dtype": "bf16", "data": "synthetic"}))


def rollouts(steps=20, warmup=3, n=5):
    from capgen.utils import rollout_captions
    cfg = preset("C2", dtype="bf16", dropout=0.3)
    vocab = {"<NULL>": 0, "<START>": 1, "<END>": 2}
    vocab.update({f"w{i}": i for i in range(3, cfg.num_vocab)})
    sd = {k: torch.from_numpy(v) for k, v in reference_init_state_dict(cfg, seed=0).items()}
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = RolloutSelfCritic(config=cfg, word_to_idx=vocab, device="cuda:0", state_dict=sd, n_samples=n,
                              baseline="greedy", seed=0)
    B, N, T = 64, 36, cfg.max_length
    f, p, c = synthetic_batch(B, N, cfg.encode_dim_features, cfg.encode_dim_positions, T, cfg.num_vocab, seed=1000)
    f = f.cuda().bfloat16()
    p = p.cuda()
    target = c[:, 1:].numpy()
    eng = m.model.engine
    caps_buf = torch.empty(n * B, T, dtype=torch.int32, device="cuda:0")
    adv_buf = torch.empty(n * B, dtype=torch.float32, device="cuda:0")
    idx = torch.arange(B, dtype=torch.int32, device="cuda:0").repeat(n)
    t = [0.0] * 4
    rew = 0.0
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, _ = eng.sample(f, p, n, 1.0, 0, i, want_logp=False)
        caps = rollout_captions(ids, m.end_idx, cfg.pad_idx)
        host = caps[..., 1:].cpu().numpy()
        t1 = time.perf_counter()
        g = rollout_captions(eng.greedy(f, p, want_attention=False)[0], m.end_idx, cfg.pad_idx)[:, 1:].cpu().numpy()
        t2 = time.perf_counter()
        r = np.stack([m.scorer.scores(target, host[j]) for j in range(n)])
        adv = r - m.scorer.scores(target, g)[None]
        t3 = time.perf_counter()
        caps_buf.copy_(caps.view(n * B, T))
        adv_buf.copy_(torch.as_tensor(adv.reshape(-1), dtype=torch.float32))
        out = eng.train_step_weighted(f, p, caps_buf, adv_buf, img_idx=idx)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        if i >= warmup:
            for k, d in enumerate((t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                t[k] += d
            rew += float(r.mean())
    ms = 1e3 * sum(t) / steps
    print(json.dumps({"metric": "roll-out SCST train images/sec (C5 shape on 1 GPU: B=64, 36x2048 feats, "
                                f"max_length={T}, n_samples={n}, greedy baseline)",
                      "value": round(B / (ms / 1e3), 1), "unit": "images/s", "ms_per_step": round(ms, 3),
                      "split_ms": dict(zip(("gpu_sample", "gpu_greedy", "host_reward", "gpu_weighted_step"),
                                           (round(1e3 * x / steps, 3) for x in t))),
                      "caption_rows_per_step": n * B, "mean_sample_reward": round(rew / steps, 5),
                      "final_loss": round(float(out.item()), 6), "tune_live_count": _lib.tune_live_count(),
                      "dtype": "bf16", "data": "synthetic"}))


if __name__ == "__main__":
    rollouts() if "--rollouts" in sys.argv[1:] else main()
