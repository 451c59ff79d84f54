"""`train()` — the training loop of main.py:25-153 over the HBM-resident input pipeline.

Cadence restated from the reference:
- every step: `MODEL.train_step` on one shuffled per-caption batch (main.py:60-67);
- every `eval_every` (100) steps: `compute_loss` on the first train and first valid batch,
  logged under `write_log` keys (main.py:69-81, WRITE_LOG of core/config.py:65-68);
- every `sample_every` (2500) steps: one greedy caption of the batch's first image next to its
  ground truths (main.py:83-102);
- per epoch: train/valid loss averaged over the zipped train/valid batches (len = the shorter
  loader, as zip() gives), greedy captions of every valid image, the candidate list written to
  `target_dir/valid.candidate.captions.pkl`, optional `evaluate(target_dir)` scores
  (main.py:104-146), and `model_{epoch}.pt` under `output_path/model/` (main.py:151).

Differences by design: batches never leave HBM (capgen.data.DeviceFeatureStore +
ResidentBatches; `train_step_resident` gathers the images inside the pack kernel), and the
TensorBoard writer / COCO evaluation (un-vendored coco-caption) are caller hooks (`log`,
`evaluate`).  The model is duck-typed: anything with the TRANSFORMER methods main.py uses.
"""
from __future__ import annotations

import contextlib
import os
import pickle

import numpy as np
import torch

from .data import DeviceFeatureStore, ResidentBatches


def _gather(store, idx):
    return store.features.index_select(0, idx.long()), store.positions.index_select(0, idx.long())


def train(model, train_split, valid_split, num_epoch, batch_size, output_path, target_dir=None,
          eval_every=100, sample_every=2500, write_log=("loss",), evaluate=None, log=print,
          device="cuda:0", feature_dtype=torch.bfloat16, seed=0, grad_clip=None, lr_schedule=None,
          weight_decay=None, ema_decay=None, eval_averaged=False, resume=None):
    """train_split / valid_split: dicts as returned by capgen.data.load_split (features,
    positions, captions, image_idxs).  Returns the per-epoch score dicts.

    grad_clip / lr_schedule (both None by default: nothing changes): handed to the model
    (`model.set_schedule`, the trainers' constructor arguments of the same names).  With clipping or
    measuring on and "grad_norm" in write_log, the step log also carries the last update's global
    gradient norm (before clipping).

    weight_decay / ema_decay (None by default, handed to the model in the same way): AdamW's decoupled
    decay and an averaged copy of the weights.  resume: a checkpoint_{epoch}.pt of an earlier run, loaded
    (`model.load_checkpoint`) before the first step, after the options above are set.  eval_averaged: the
    per-epoch evaluation (losses and greedy captions) runs inside `model.averaged()`, and the averaged
    weights are also written as model_{epoch}.ema.pt.  With any of these four set, checkpoint_{epoch}.pt
    (`model.save_checkpoint`) is written beside model_{epoch}.pt.  With the defaults nothing changes."""
    new_options = weight_decay is not None or ema_decay is not None or eval_averaged or resume is not None
    if weight_decay is not None or ema_decay is not None:
        model.set_schedule(lr_schedule=lr_schedule, grad_clip=grad_clip, weight_decay=weight_decay,
                           ema_decay=ema_decay)
    elif grad_clip is not None or lr_schedule is not None:
        model.set_schedule(lr_schedule=lr_schedule, grad_clip=grad_clip)
    if resume is not None:
        model.load_checkpoint(resume)
    if eval_averaged and ema_decay is None:
        # (a stand-in model without an engine cannot be asked; a real one fails here, not after an epoch)
        eng = getattr(getattr(model, "model", None), "engine", None)
        if eng is not None and eng.ema_info()[0] == 0.0:
            raise ValueError("capgen train: eval_averaged needs an average -- pass ema_decay, or resume from a "
                             "checkpoint that holds one")
    log_norm = "grad_norm" in write_log
    write_log = tuple(k for k in write_log if k != "grad_norm")  # (not a compute_loss key)
    model_dir = os.path.join(output_path, "model")
    os.makedirs(model_dir, exist_ok=True)
    target_dir = target_dir or os.path.join(output_path, "valid")
    os.makedirs(target_dir, exist_ok=True)

    stores, loaders = {}, {}
    for name, split, shuffle in (("train", train_split, True), ("valid", valid_split, False)):
        stores[name] = DeviceFeatureStore(split["features"], split["positions"], device=device, dtype=feature_dtype)
        loaders[name] = ResidentBatches(split["captions"], split["image_idxs"], batch_size, device=device,
                                        shuffle=shuffle, seed=seed)
    # the fixed evaluation batches: the first train (shuffled) and valid batch (main.py:45-55)
    eval_batches = {n: next(iter(loaders[n])) for n in ("train", "valid")}
    n_valid_images = stores["valid"].n_images
    train_caps = np.asarray(train_split["captions"])
    train_img = np.asarray(train_split["image_idxs"])

    def loss_of(name, idx, caps):
        f, p = _gather(stores[name], idx)
        return model.compute_loss(object_features=f, position_features=p, target_caption=caps)

    n_iter = len(loaders["train"])
    history = []
    for epoch in range(1, num_epoch + 1):
        log(f"Epoch {epoch}")
        for i, (idx, caps) in enumerate(loaders["train"]):
            model.train_step_resident(stores["train"], idx, caps)
            step = i + n_iter * (epoch - 1)
            if (i + 1) % eval_every == 0:
                tl = loss_of("train", *eval_batches["train"])
                vl = loss_of("valid", *eval_batches["valid"])
                entry = {"step": step, **{k: {"train": tl[k].mean().item(), "valid": vl[k].mean().item()}
                                          for k in write_log}}
                eng = getattr(getattr(model, "model", None), "engine", None)
                if log_norm and getattr(eng, "grad_clip", None):
                    entry["grad_norm"] = eng.grad_norm()
                log(entry)
            if (i + 1) % sample_every == 0:
                f, p = _gather(stores["train"], idx[:1])
                sample, _ = model.generate_caption(object_features=f, position_features=p)
                img = int(idx[0].item())
                truths = model.decode_captions(train_caps[train_img == img])
                log({"step": step, "sample": sample[0], "truths": truths})

        # evaluation (main.py:104-146)
        valid_caption = [""] * n_valid_images
        logs = {k: {"train": 0.0, "valid": 0.0} for k in write_log}
        with model.averaged() if eval_averaged else contextlib.nullcontext():
            for (t_idx, t_caps), (v_idx, v_caps) in zip(loaders["train"], loaders["valid"]):
                tl = loss_of("train", t_idx, t_caps)
                vl = loss_of("valid", v_idx, v_caps)
                for k in write_log:
                    logs[k]["train"] += tl[k].mean().item()
                    logs[k]["valid"] += vl[k].mean().item()
                f, p = _gather(stores["valid"], v_idx)
                captions, _ = model.generate_caption(object_features=f, position_features=p)
                for j, c in zip(v_idx.tolist(), captions):
                    valid_caption[j] = c
            if eval_averaged:  # (save() writes the parameter arena: the average, in here)
                model.save(path=os.path.join(model_dir, f"model_{epoch}.ema.pt"))
        # the reference divides by len(valid_dataloader) (main.py:130-132)
        for k in write_log:
            logs[k]["train"] /= max(1, len(loaders["valid"]))
            logs[k]["valid"] /= max(1, len(loaders["valid"]))
        with open(os.path.join(target_dir, "valid.candidate.captions.pkl"), "wb") as fh:
            pickle.dump(valid_caption, fh)
        scores = dict(evaluate(target_dir) if evaluate is not None else {})
        scores.update(logs)
        log({"epoch": epoch, "train_loss": scores["loss"]["train"] if "loss" in scores else None,
             "valid_loss": scores["loss"]["valid"] if "loss" in scores else None})
        model.save(path=os.path.join(model_dir, f"model_{epoch}.pt"))
        if new_options:
            model.save_checkpoint(os.path.join(model_dir, f"checkpoint_{epoch}.pt"))
        history.append(scores)
    return history
