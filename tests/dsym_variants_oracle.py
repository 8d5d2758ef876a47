"""float64 numpy oracle of the front ends of DiscreteSymbolDurationGenerator and
DiscreteSymbolF0Generator (reference models/hifigan.py:1100-1487, layers/duration_predictor.py,
layers/length_regulator.py). The body is oracle.melgan_numpy.hifigan_forward. ``sd`` is a
weight-norm-folded state dict of float32 arrays; everything is computed in float64 from them."""

import numpy as np


def _f64(sd, key):
    return np.asarray(sd[key], np.float64)


def predictor_log_durations(x, sd, prefix="duration_predictor."):
    """DurationPredictor.forward on one utterance: x (T, idim) -> (T,) log durations.
    n x [Conv1d(k, zero 'same' padding) -> ReLU -> LayerNorm over channels (eps 1e-12)] -> Linear."""
    h = np.asarray(x, np.float64)
    i = 0
    while f"{prefix}conv.{i}.0.weight" in sd:
        w, b = _f64(sd, f"{prefix}conv.{i}.0.weight"), _f64(sd, f"{prefix}conv.{i}.0.bias")
        k = w.shape[2]
        p = (k - 1) // 2
        hp = np.pad(h, ((p, p), (0, 0)))
        T = h.shape[0]
        y = np.zeros((T, w.shape[0]))
        for tap in range(k):
            y += hp[tap:tap + T] @ w[:, :, tap].T
        y = np.maximum(y + b, 0.0)
        mean = y.mean(1, keepdims=True)
        var = ((y - mean) ** 2).mean(1, keepdims=True)
        h = (y - mean) / np.sqrt(var + 1e-12) * _f64(sd, f"{prefix}conv.{i}.2.weight") + _f64(sd, f"{prefix}conv.{i}.2.bias")
        i += 1
    return h @ _f64(sd, prefix + "linear.weight").reshape(-1) + float(_f64(sd, prefix + "linear.bias").reshape(-1)[0])


def durations(log_d, offset=1.0):
    """DurationPredictor.inference: clamp(round(exp(x) - offset), min=0).long(), round half to even."""
    v = np.rint(np.exp(np.asarray(log_d, np.float64)) - offset)
    return np.where(np.isnan(v), 0.0, np.maximum(v, 0.0)).astype(np.int64)  # (a NaN becomes 0)


def regulate(rows, ds, total=None):
    """LengthRegulator on one utterance: rows (T, D) repeated ds[t] times each; all-zero durations
    count as all ones; zero rows up to ``total`` rows (pad_list)."""
    ds = np.asarray(ds, np.int64)
    if ds.sum() == 0:
        ds = np.ones_like(ds)
    out = np.repeat(np.asarray(rows), ds, axis=0)
    if total is not None and total > out.shape[0]:
        out = np.concatenate([out, np.zeros((total - out.shape[0], out.shape[1]), out.dtype)])
    return out


def table_weights(sd, fixed):
    """The weighted-sum weights as the reference normalises them in fp32 (softmax unless fixed)."""
    w = np.asarray(sd["weights"], np.float32)
    if fixed:
        return w
    import torch

    return torch.nn.functional.softmax(torch.from_numpy(w), dim=-1).numpy()


def token_features(ids, sd, g=None, weights=None):
    """(T, dim) float64: emb[ids] (+ spk_emb[g]), or with ``weights`` (L,) and ids (T, L) the sum
    over tables emb.l of weights[l] * emb_l[ids[:, l]]."""
    ids = np.asarray(ids, np.int64)
    if weights is not None:
        return sum(float(weights[l]) * _f64(sd, f"emb.{l}.weight")[ids[:, l]] for l in range(len(weights)))
    f = _f64(sd, "emb.weight")[ids]
    if g is not None:
        # (the reference adds in fp32; the sum of two fp32 values is within 2^-24 relative of this)
        f = f + _f64(sd, "spk_emb.weight")[g]
    return f


def f0_features(f0, sd):
    """f0_embedding = Linear(1, lin): (T,) -> (T, lin) float64."""
    return np.asarray(f0, np.float64)[:, None] * _f64(sd, "f0_embedding.weight").reshape(1, -1) + _f64(sd, "f0_embedding.bias")


def body(feats, sd, params):
    """feats (T, C) -> (T * hop, out_channels) through the HiFiGAN body."""
    from oracle import melgan_numpy

    body_params = {k: params[k] for k in ("out_channels", "channels", "kernel_size", "upsample_scales",
                                           "upsample_kernel_sizes", "resblock_kernel_sizes", "resblock_dilations",
                                           "use_additional_convs", "nonlinear_activation_params") if k in params}
    return melgan_numpy.hifigan_forward(np.asarray(feats, np.float64).T, sd, body_params).T


def duration_generator(ids, sd, params, ds=None, total=None):
    """One utterance of DiscreteSymbolDurationGenerator: ids (T,) -> (audio (sum(ds) * hop, out),
    log durations (T,), durations used (T,))."""
    rows = _f64(sd, "emb.weight")[np.asarray(ids, np.int64)]
    log_d = predictor_log_durations(rows, sd)
    used = durations(log_d, params.get("duration_offset", 1.0)) if ds is None else np.asarray(ds, np.int64)
    return body(regulate(rows, used, total), sd, params), log_d, used


def f0_generator(ids, sd, params, f0=None, g=None):
    """One utterance of DiscreteSymbolF0Generator: ids (T,) or (T, L) -> audio (T * hop, out)."""
    w = table_weights(sd, params.get("use_fix_weight", False)) if params.get("use_weight_sum") else None
    feats = token_features(ids if w is not None else np.asarray(ids).reshape(len(ids), -1)[:, 0], sd, g, w)
    if params.get("use_f0", True):
        feats = np.concatenate([feats, f0_features(f0, sd)], 1)
    return body(feats, sd, params)
