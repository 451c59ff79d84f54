"""Generate the golden fixtures from the REFERENCE implementation (build container only).

Run:  python tests/golden/gen_golden.py        (needs /root/reference; not run on the GPU box)

It imports shao-chi/Image-Caption's `core.TRANSFORMER.model.Transformer` from
/root/reference with two un-vendored imports stubbed (coco-caption's
`core.metrics.*`, imported by loss.py:7-9 but unused on this path, and `hickle`,
imported by core/utils.py:7), loads the deterministic fixture weights
(capgen.params.fixture_state_dict), and records, in eval mode (dropout off):
  * loss and full logits of Transformer.forward (model.py:79-98; logits via a hook
    on `classifer`),
  * per-parameter gradient sums / abs-sums / sampled values after loss.backward(),
  * the loss after a second Adam(lr) step and per-parameter deltas after two steps
    (models.py:111-126),
  * greedy ids + attention_list (model.py:101-132) and beam-5 ids (model.py:135-200);
  * PolicyNetwork greedy / beam ids (model_RL.py:100-199: log-softmax scoring).
Only inputs and outputs are written (tests/golden/*.npz); the reference source never
leaves this container.
"""
from __future__ import annotations

import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "image-caption_amd"))

from capgen.config import preset  # noqa: E402
from capgen.params import fixture_state_dict, reference_param_specs  # noqa: E402
from capgen.synthetic import synthetic_batch  # noqa: E402

REF = "/root/reference"
N_SAMPLES = 8


def import_reference():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    for name in ["hickle", "core.metrics", "core.metrics.cider", "core.metrics.cider.cider",
                 "core.metrics.ciderD", "core.metrics.ciderD.ciderD", "core.metrics.bleu",
                 "core.metrics.bleu.bleu"]:
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["core.metrics.cider.cider"].Cider = object
    sys.modules["core.metrics.ciderD.ciderD"].CiderD = object
    sys.modules["core.metrics.bleu.bleu"].Bleu = object
    from core.TRANSFORMER.model import Transformer
    return Transformer


def sample_index(name, numel):
    r = np.random.default_rng(zlib.crc32(name.encode()))
    return np.sort(r.choice(numel, size=min(N_SAMPLES, numel), replace=False))


def build(Transformer, cfg):
    return Transformer(
        num_vocab=cfg.num_vocab, max_length=cfg.max_length,
        encode_dim_positions=cfg.encode_dim_positions, encode_dim_features=cfg.encode_dim_features,
        device="cpu", output_name=cfg.output_name, encode_mask=cfg.encode_mask, pad_idx=cfg.pad_idx,
        dropout=cfg.dropout, encode_input_size=cfg.encode_input_size, encode_q_k_dim=cfg.encode_q_k_dim,
        encode_v_dim=cfg.encode_v_dim, encode_hidden_size=cfg.encode_hidden_size,
        encode_num_blocks=cfg.encode_num_blocks, encode_num_heads=cfg.encode_num_heads,
        dim_word_embedding=cfg.dim_word_embedding, decode_input_size=cfg.decode_input_size,
        decode_q_k_dim=cfg.decode_q_k_dim, decode_v_dim=cfg.decode_v_dim,
        decode_hidden_size=cfg.decode_hidden_size, decode_num_blocks=cfg.decode_num_blocks,
        decode_num_heads=cfg.decode_num_heads, split_position=cfg.split_position,
        split_image_objects=cfg.split_image_objects, move_first_image_feature=cfg.move_first_image_feature)


def make_fixture(tag, cfg, B, N, T, seed, beam_k=5, min_valid=None):
    Transformer = import_reference()
    torch.manual_seed(0)
    model = build(Transformer, cfg)
    sd = {k: torch.from_numpy(v) for k, v in fixture_state_dict(cfg, seed=seed).items()}
    model.load_state_dict(sd, strict=True)
    model.eval()
    feats, pos, caps = synthetic_batch(B, N, cfg.encode_dim_features, cfg.encode_dim_positions,
                                       T, cfg.num_vocab, seed=seed + 100, min_valid=min_valid)
    out = {"feats": feats.numpy(), "pos": pos.numpy(), "caps": caps.numpy()}

    logits_box = {}
    h = model.classifer.register_forward_hook(lambda m, i, o: logits_box.__setitem__("x", o.detach()))
    opt = torch.optim.Adam((p for p in model.parameters() if p.requires_grad), lr=cfg.learning_rate)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}

    opt.zero_grad()
    loss = model(object_features=feats, position_features=pos, target_caption=caps)["loss"]
    loss.backward()
    out["loss"] = np.float64(loss.item())
    out["logits"] = logits_box["x"].numpy()
    names = [n for n, _ in reference_param_specs(cfg)]
    params = dict(model.named_parameters())
    assert sorted(names) == sorted(params), "param spec drift vs reference"
    gsum, gabs, gsamp = [], [], []
    for n in names:
        g = params[n].grad.detach().double().reshape(-1)
        gsum.append(g.sum().item())
        gabs.append(g.abs().sum().item())
        gsamp.append(g[sample_index(n, g.numel())].numpy())
    out["grad_sum"], out["grad_abs"] = np.array(gsum), np.array(gabs)
    out["grad_samples"] = np.concatenate(gsamp)
    opt.step()
    opt.zero_grad()
    loss2 = model(object_features=feats, position_features=pos, target_caption=caps)["loss"]
    loss2.backward()
    opt.step()
    out["loss_after_step1"] = np.float64(loss2.item())
    dsum, dabs, dsamp = [], [], []
    for n in names:
        dlt = (params[n].detach() - before[n]).double().reshape(-1)
        dsum.append(dlt.sum().item())
        dabs.append(dlt.abs().sum().item())
        dsamp.append(dlt[sample_index(n, dlt.numel())].numpy())
    out["delta2_sum"], out["delta2_abs"] = np.array(dsum), np.array(dabs)
    out["delta2_samples"] = np.concatenate(dsamp)
    h.remove()

    model.load_state_dict(sd, strict=True)
    model.eval()
    ids, attn = model.generate_caption_vector(object_features=feats, position_features=pos)
    out["greedy_ids"] = ids.numpy()
    out["greedy_attn"] = np.stack(attn).astype(np.float32)
    if beam_k:
        out["beam_ids"] = model.beam_search(object_features=feats, position_features=pos,
                                            beam_size=beam_k).numpy()
        out["beam_k"] = np.int64(beam_k)
    out["seed"] = np.int64(seed)
    out["cfg"] = np.array(repr(cfg))
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: loss={out['loss']:.6f} loss_after_step1={out['loss_after_step1']:.6f}")


# ---- SCST (SelfCriticNetwork, models.py:137-211; model_RL.py:75-97; loss.py:31-220) -------
# CIDEr-D / BLEU / self-CIDEr live in the un-vendored coco-caption code (core.metrics.*), so
# the scorers are stubbed with INJECTED per-image scores (C5 parity is pinned
# for the loss mechanics given reward vectors).  Weights: core/config.py:81-85.
RL_WEIGHTS = dict(structure_loss_weight=0.5, cider_reward_weight=1.0, bleu_reward_weight=1.0,
                  entropy_reward_weight=1.0, self_cider_reward_weight=1.0)


def make_rl_fixture(tag, cfg, B, N, T, seed, min_valid=None, pad_frac=0.0, store_inputs=True,
                    store_relu_masks=False):
    """pad_frac > 0: raise the classifier bias of the pad id so that about that fraction of the
    argmax samples are 0 (exercises the structure-loss mask; the boost is stored as
    `pad_bias_boost` and applied to the fixture weights by the tests).  store_inputs=False (the
    full C5 shape): the batch is not stored -- the tests regenerate it with
    capgen.synthetic.synthetic_batch from the recorded (B, N, T, V, seed, min_valid)."""
    import pickle
    import tempfile
    import_reference()
    rng = np.random.default_rng(seed + 7)
    cider = rng.uniform(0.0, 2.0, size=B)
    bleu = rng.uniform(0.0, 1.0, size=B)

    class StubCiderD:
        def __init__(self, df=None):
            pass

        def compute_score(self, gts, res):
            assert len(res) == B
            return float(cider.mean()), cider.copy()

    class StubBleu:
        def __init__(self, n=4, print_=False):
            pass

        def compute_score(self, gts, res):
            return [0.0] * 4, [list(bleu) for _ in range(4)]

    class StubCider:
        def __init__(self, df=None):
            pass

        def my_self_cider(self, res):
            return [np.array([[4.0]])]  # one caption per image: a 1x1 kernel -> diversity term 0

    sys.modules["core.metrics.ciderD.ciderD"].CiderD = StubCiderD
    sys.modules["core.metrics.bleu.bleu"].Bleu = StubBleu
    sys.modules["core.metrics.cider.cider"].Cider = StubCider
    for m in [k for k in list(sys.modules) if k.startswith("core.TRANSFORMER.loss")]:
        del sys.modules[m]
    from core.TRANSFORMER.loss import ReinforcementLearningLoss
    from core.TRANSFORMER.model_RL import PolicyNetwork

    torch.manual_seed(0)
    model = PolicyNetwork(
        num_vocab=cfg.num_vocab, max_length=cfg.max_length, encode_dim_positions=cfg.encode_dim_positions,
        encode_dim_features=cfg.encode_dim_features, device="cpu", pad_idx=cfg.pad_idx, dropout=cfg.dropout,
        encode_mask=cfg.encode_mask, encode_input_size=cfg.encode_input_size, encode_q_k_dim=cfg.encode_q_k_dim,
        encode_v_dim=cfg.encode_v_dim, encode_hidden_size=cfg.encode_hidden_size,
        encode_num_blocks=cfg.encode_num_blocks, encode_num_heads=cfg.encode_num_heads,
        dim_word_embedding=cfg.dim_word_embedding, decode_input_size=cfg.decode_input_size,
        decode_q_k_dim=cfg.decode_q_k_dim, decode_v_dim=cfg.decode_v_dim,
        decode_hidden_size=cfg.decode_hidden_size, decode_num_blocks=cfg.decode_num_blocks,
        decode_num_heads=cfg.decode_num_heads)
    sd = {k: torch.from_numpy(v) for k, v in fixture_state_dict(cfg, seed=seed).items()}
    model.load_state_dict(sd, strict=True)
    model.eval()
    feats, pos, caps = synthetic_batch(B, N, cfg.encode_dim_features, cfg.encode_dim_positions,
                                       T, cfg.num_vocab, seed=seed + 100, min_valid=min_valid)
    boost = 0.0
    if pad_frac > 0:
        with torch.no_grad():
            lg = model(object_features=feats, position_features=pos, target_caption=caps)
            gap = lg[..., 1:].max(-1).values - lg[..., 0]
            boost = float(torch.quantile(gap.reshape(-1), pad_frac)) + 1e-3
        sd["classifer.bias"] = sd["classifer.bias"].clone()
        sd["classifer.bias"][0] += boost
        model.load_state_dict(sd, strict=True)
    vocab = {"<NULL>": 0, "<START>": 1, "<END>": 2}
    vocab.update({f"w{i}": i for i in range(3, cfg.num_vocab)})
    with tempfile.NamedTemporaryFile(suffix=".pkl", delete=False) as fh:
        pickle.dump(vocab, fh)
        vocab_path = fh.name
    crit = ReinforcementLearningLoss(word_to_idx_path=vocab_path, pad_idx=cfg.pad_idx, **RL_WEIGHTS)
    os.unlink(vocab_path)

    out = {"inj_cider": cider, "inj_bleu": bleu, "pad_bias_boost": np.float64(boost)}
    if store_inputs:
        out.update(feats=feats.numpy(), pos=pos.numpy(), caps=caps.numpy())
    else:
        out.update(batch_shape=np.array([B, N, T, cfg.num_vocab]), batch_seed=np.int64(seed + 100),
                   batch_min_valid=np.int64(-1 if min_valid is None else min_valid))
    for k, v in RL_WEIGHTS.items():
        out[k] = np.float64(v)
    hooks = []
    if store_relu_masks:
        # the ReLU pattern the reference differentiates: a pre-activation within fp32 rounding of zero
        # lands on either side depending on the host's GEMM kernels, and one such unit moves whole
        # gradient tensors by more than the tests' bound, so the pattern is part of the recorded result
        def record(prefix):
            def hook(m, i, o):
                out[f"relu_mask.{prefix}"] = np.packbits((o.detach() > 0).numpy().reshape(-1))
                out[f"relu_shape.{prefix}"] = np.array(o.shape, dtype=np.int64)
            return hook
        for name, mod in model.named_modules():
            if name.endswith(".feed_forward.position_wise_1"):
                hooks.append(mod.register_forward_hook(record(name[:-len(".position_wise_1")])))
    logits = model(object_features=feats, position_features=pos, target_caption=caps)
    for h in hooks:
        h.remove()
    seq, logp = model.sample(output=logits)
    loss = crit(model_output=logits.cpu(), sample_sequence=seq.cpu(), sample_logprobs=logp.cpu(), target=caps)
    loss["loss"].mean().backward()
    out["loss"] = np.float64(loss["loss"].item())
    out["language_model_loss"] = np.float64(loss["language_model_loss"].item())
    out["structure_loss"] = np.float64(loss["structure_loss"].item())
    out["reward"] = loss["reward"].detach().numpy().reshape(-1)
    out["sample"] = seq.numpy()
    names = [n for n, _ in reference_param_specs(cfg)]
    params = dict(model.named_parameters())
    gsum, gabs, gsamp = [], [], []
    for n in names:
        g = params[n].grad.detach().double().reshape(-1)
        gsum.append(g.sum().item())
        gabs.append(g.abs().sum().item())
        gsamp.append(g[sample_index(n, g.numel())].numpy())
    out["grad_sum"], out["grad_abs"] = np.array(gsum), np.array(gabs)
    out["grad_samples"] = np.concatenate(gsamp)
    out["seed"] = np.int64(seed)
    out["cfg"] = np.array(repr(cfg))
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: loss={out['loss']:.6f} lm={out['language_model_loss']:.6f} "
          f"struct={out['structure_loss']:.6f}")


def build_policy(PolicyNetwork, cfg):
    return PolicyNetwork(
        num_vocab=cfg.num_vocab, max_length=cfg.max_length, encode_dim_positions=cfg.encode_dim_positions,
        encode_dim_features=cfg.encode_dim_features, device="cpu", pad_idx=cfg.pad_idx, dropout=cfg.dropout,
        encode_mask=cfg.encode_mask, encode_input_size=cfg.encode_input_size, encode_q_k_dim=cfg.encode_q_k_dim,
        encode_v_dim=cfg.encode_v_dim, encode_hidden_size=cfg.encode_hidden_size,
        encode_num_blocks=cfg.encode_num_blocks, encode_num_heads=cfg.encode_num_heads,
        dim_word_embedding=cfg.dim_word_embedding, decode_input_size=cfg.decode_input_size,
        decode_q_k_dim=cfg.decode_q_k_dim, decode_v_dim=cfg.decode_v_dim,
        decode_hidden_size=cfg.decode_hidden_size, decode_num_blocks=cfg.decode_num_blocks,
        decode_num_heads=cfg.decode_num_heads)


def make_policy_decode_fixture(tag, cfg, B, N, T, seed, beam_k, min_valid=None):
    """PolicyNetwork decoding (model_RL.py:100-199): greedy = argmax of LogSoftmax, beam search
    accumulates LOG-probabilities (model_RL.py:72,157,182) -- unlike Transformer.beam_search,
    which adds probabilities.  Also records Transformer.beam_search on the same weights/inputs,
    so the fixture shows the two rules choosing different beams."""
    Transformer = import_reference()
    from core.TRANSFORMER.model_RL import PolicyNetwork
    torch.manual_seed(0)
    model = build_policy(PolicyNetwork, cfg)
    sd = {k: torch.from_numpy(v) for k, v in fixture_state_dict(cfg, seed=seed).items()}
    model.load_state_dict(sd, strict=True)
    model.eval()
    feats, pos, caps = synthetic_batch(B, N, cfg.encode_dim_features, cfg.encode_dim_positions,
                                       T, cfg.num_vocab, seed=seed + 100, min_valid=min_valid)
    out = {"feats": feats.numpy(), "pos": pos.numpy(), "caps": caps.numpy()}
    ids, attn = model.generate_caption_vector(object_features=feats, position_features=pos)
    out["greedy_ids"] = ids.numpy()
    out["greedy_attn"] = np.stack(attn).astype(np.float32)
    out["beam_ids"] = model.beam_search(object_features=feats, position_features=pos, beam_size=beam_k).numpy()
    out["beam_k"] = np.int64(beam_k)
    tr = build(Transformer, cfg)
    tr.load_state_dict(sd, strict=True)
    tr.eval()
    out["transformer_beam_ids"] = tr.beam_search(object_features=feats, position_features=pos,
                                                 beam_size=beam_k).numpy()
    out["seed"] = np.int64(seed)
    out["cfg"] = np.array(repr(cfg))
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **out)
    ndiff = int((out["beam_ids"] != out["transformer_beam_ids"]).any(1).sum())
    print(f"wrote {path}: {ndiff}/{B} images decode differently under the Transformer (probability) beam")


POLICY_FIXTURES = {
    # tag: (cfg, B, N, T, seed, beam_k, min_valid)
    "c1_policy": (preset("C1"), 8, 8, 10, 9, 5, 4),
    "c2s_policy": (preset("C2", num_vocab=1000), 2, 36, 20, 10, 5, 12),
}


RL_FIXTURES = {
    # tag: (cfg, B, N, T, seed, min_valid, pad_frac)
    "c5_rl": (preset("C1"), 8, 8, 10, 5, 4, 0.0),
    "c5_rl_pad": (preset("C1"), 8, 8, 10, 6, 4, 0.35),
    # the C5 model itself (6+6 blocks, d=512, h=8, 36 regions, T=20) at the c2s vocabulary
    "c5_rl_c2s": (preset("C2", num_vocab=1000), 4, 36, 20, 12, 12, 0.2),
}
# fixtures that also record the reference's ReLU pattern (relu_mask.<feed_forward prefix>, bit-packed):
# c5_rl_c2s has a unit in encoder block 4 whose pre-activation is 5.9e-7 in float64 and whose sign
# alone moves encoder.encoder.2's q_linear gradient by 2.2e-4 of its abs-sum
RL_RELU_MASKS = {"c5_rl_c2s"}
# C5's own shape (SCST on the C2 model, 64 images per GPU, V=10000); inputs regenerated
RL_FIXTURES_SEEDED = {
    "c5_rl_c5": (preset("C2"), 64, 36, 20, 13, None, 0.2),
}


FIXTURES = {
    # tag: (cfg, B, N, T, seed, beam_k, min_valid)
    "c1": (preset("C1"), 8, 8, 10, 0, 5, 4),
    "c1_encmask": (preset("C1", encode_mask=True), 4, 8, 10, 1, 3, 4),
    "c1_focal": (preset("C1", output_name="FocalLoss_Transformer"), 4, 8, 10, 2, 0, 4),
    "c2s": (preset("C2", num_vocab=1000), 2, 36, 20, 3, 5, 12),
    "c1_splitpos": (preset("C1", split_position=True), 4, 8, 10, 4, 3, 4),
    "c1_imgobj": (preset("C1", split_image_objects=True), 4, 8, 10, 7, 3, 4),
    "c1_movefirst": (preset("C1", move_first_image_feature=True), 4, 8, 10, 8, 3, 4),
}


def main(tags=None):
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    for tag, (cfg, B, N, T, seed, k, mv) in FIXTURES.items():
        if tags and tag not in tags:
            continue
        make_fixture(tag, cfg, B, N, T, seed, beam_k=k, min_valid=mv)
    for tag, (cfg, B, N, T, seed, k, mv) in POLICY_FIXTURES.items():
        if tags and tag not in tags:
            continue
        make_policy_decode_fixture(tag, cfg, B, N, T, seed, k, min_valid=mv)
    for tag, (cfg, B, N, T, seed, mv, pf) in RL_FIXTURES.items():
        if tags and tag not in tags:
            continue
        make_rl_fixture(tag, cfg, B, N, T, seed, min_valid=mv, pad_frac=pf, store_relu_masks=tag in RL_RELU_MASKS)
    for tag, (cfg, B, N, T, seed, mv, pf) in RL_FIXTURES_SEEDED.items():
        if tags and tag not in tags:
            continue
        make_rl_fixture(tag, cfg, B, N, T, seed, min_valid=mv, pad_frac=pf, store_inputs=False)


if __name__ == "__main__":
    main(sys.argv[1:])
