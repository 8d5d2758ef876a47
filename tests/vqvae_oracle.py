"""The project's own torch-CPU restatement of VQVAE (parallel_wavegan/models/vqvae.py:16-171 with a
MelGANDiscriminator encoder, models/melgan.py:260-396, and functions/vector_quantizer.py:32-52), in
fp32 or float64, over a folded state dict; and the index parity rule the CPU and GPU tests share.
The decoder is the MelGAN oracle (oracle/melgan_torch_cpu.py in fp32, restated here for float64).
Not a test module."""

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24


def fixture_codebook(table, code_scale, shift=None, dup=None, dup_swap=None):
    """The codebook of a fixture from the seeded N(0, 1) table: scaled to the spread of the encoder
    output around ``shift`` (the bias of the encoder's last conv, where its outputs centre; None
    without biases) and moved there; for the ``dup`` case row ``dup_swap`` (the code the reference uses most) is first exchanged with
    row dup[0], then row dup[0] is copied over row dup[1]."""
    book = np.asarray(table, np.float32) * np.float32(code_scale)
    if shift is not None:
        book = book + np.asarray(shift, np.float32)[None, :]
    if dup:
        if dup_swap is not None:
            book[[dup[0], dup_swap]] = book[[dup_swap, dup[0]]]
        book[dup[1]] = book[dup[0]]
    return book


def codebook_shift(sd):
    """The bias of the encoder's last conv in a (folded or weight-norm) state dict, None without one."""
    keys = [k for k in sd if k.startswith("encoder.layers.") and k.endswith(".bias")]
    return np.asarray(sd[max(keys, key=lambda k: int(k.split(".")[2]))], np.float32) if keys else None


def _t(sd, key, dtype):
    return torch.from_numpy(np.asarray(sd[key])).to(dtype)


def encoder(x, sd, conf, dtype=torch.float64, prefix="encoder.", taps=None):
    """x (T,) -> z_e (T', out_channels); ``taps``: a list that receives every layer's (T_i, C_i) output."""
    ks = conf.get("kernel_sizes", [5, 3])
    scales = conf["downsample_scales"]
    slope = conf.get("nonlinear_activation_params", {"negative_slope": 0.2})["negative_slope"]
    bias = conf.get("bias", True)
    h = torch.as_tensor(np.asarray(x)).to(dtype).view(1, 1, -1)

    def b(key):
        return _t(sd, prefix + key, dtype) if bias else None

    k0 = int(np.prod(ks))
    h = F.leaky_relu(F.conv1d(F.pad(h, ((k0 - 1) // 2,) * 2, mode="reflect"), _t(sd, prefix + "layers.0.1.weight", dtype),
                              b("layers.0.1.bias")), slope)
    if taps is not None:
        taps.append(h[0].T)
    for i, s in enumerate(scales):
        w = _t(sd, prefix + f"layers.{1 + i}.0.weight", dtype)
        h = F.leaky_relu(F.conv1d(h, w, b(f"layers.{1 + i}.0.bias"), stride=s, padding=5 * s, groups=h.size(1) // 4), slope)
        if taps is not None:
            taps.append(h[0].T)
    n = len(scales) + 1
    h = F.leaky_relu(F.conv1d(h, _t(sd, prefix + f"layers.{n}.0.weight", dtype), b(f"layers.{n}.0.bias"),
                              padding=(ks[0] - 1) // 2), slope)
    h = F.conv1d(h, _t(sd, prefix + f"layers.{n + 1}.weight", dtype), b(f"layers.{n + 1}.bias"), padding=(ks[1] - 1) // 2)
    return h[0].T.contiguous()


def distances(z, book):
    """functions/vector_quantizer.py:36-46: addmm(||e||^2 + ||z||^2, z, e^T, alpha=-2)."""
    book_sqr = torch.sum(book ** 2, dim=1)
    z_sqr = torch.sum(z ** 2, dim=1, keepdim=True)
    return torch.addmm(book_sqr + z_sqr, z, book.t(), alpha=-2.0, beta=1.0)


def nearest(z, book):
    return torch.min(distances(z, book), dim=1)[1]


def decoder_rows(idx, l, g, sd, dtype=torch.float64):
    """[codebook[idx] ; local_embed(l) ; global_embed[g]] as (T', width); l (T', num_local) or None."""
    parts = [_t(sd, "codebook.embedding.weight", dtype)[torch.as_tensor(np.asarray(idx)).long()]]
    if l is not None:
        l = torch.as_tensor(np.asarray(l)).to(dtype)
        if "local_embed.weight" in sd:
            l = F.conv1d(l.T.unsqueeze(0), _t(sd, "local_embed.weight", dtype), _t(sd, "local_embed.bias", dtype))[0].T
        parts.append(l)
    if g is not None:
        parts.append(_t(sd, "global_embed.weight", dtype)[int(g)].expand(parts[0].size(0), -1))
    return torch.cat(parts, dim=1)


def melgan_decoder(c, sd, conf, dtype=torch.float64, prefix="decoder."):
    """MelGANGenerator (models/melgan.py:17-170, layers/residual_stack.py) over c (T', in) -> (T' * hop, 1),
    default activation / padding choices (LeakyReLU 0.2, ReflectionPad1d, final tanh)."""
    scales, stacks = conf["upsample_scales"], conf.get("stacks", 3)
    ks, sk = conf.get("kernel_size", 7), conf.get("stack_kernel_size", 3)

    def conv(h, i, pad, dil=1, sub=""):
        key = f"{prefix}melgan.{i}{sub}"
        if pad:
            h = F.pad(h, (pad, pad), mode="reflect")
        return F.conv1d(h, _t(sd, key + ".weight", dtype), _t(sd, key + ".bias", dtype), dilation=dil)

    h = torch.as_tensor(np.asarray(c)).to(dtype).T.unsqueeze(0)
    h = conv(h, 1, (ks - 1) // 2)
    i = 2
    for s in scales:
        key = f"{prefix}melgan.{i + 1}"
        h = F.conv_transpose1d(F.leaky_relu(h, 0.2), _t(sd, key + ".weight", dtype), _t(sd, key + ".bias", dtype),
                               stride=s, padding=s // 2 + s % 2, output_padding=s % 2)
        i += 2
        for j in range(stacks):
            d = sk ** j
            t = conv(F.leaky_relu(h, 0.2), i, (sk - 1) // 2 * d, d, ".stack.2")
            t = conv(F.leaky_relu(t, 0.2), i, 0, 1, ".stack.4")
            h = t + conv(h, i, 0, 1, ".skip_layer")
            i += 1
    h = torch.tanh(conv(F.leaky_relu(h, 0.2), i + 2, (ks - 1) // 2))
    return h[0].T.contiguous()


# ---------------------------------------------------------------------------------------------- index rule
def index_rule(z_e, book, idx, ref_idx=None, z_used=None):
    """The index parity rule. d64: float64 distances from the fixture's z_e (rows x D) to the codebook,
    k* their arg-min, tau_r = 2 (D + 2) u (||z_r|| + max_k ||e_k||)^2. A returned index k must satisfy
    d64[r, k] - d64[r, k*] <= allowance_r, where the allowance is tau_r for the kernel test and
    tau_r + 2 ||z_used_r - z_e_r|| ||e_k - e_k*|| when the search ran on ``z_used`` (the GPU encoder's
    output). Returns (violations, frames under their allowance, mismatches against ``ref_idx`` on rows whose
    float64 margin exceeds the allowance). Exact copies of a code row count as one code whose index is
    the lowest of the copies (the tie rule), so a copy never makes a frame "under its allowance"."""
    z = np.asarray(z_e, np.float64)
    e = np.asarray(book, np.float64)
    idx = np.asarray(idx).astype(np.int64).reshape(-1)
    rows, D = z.shape
    d = (z ** 2).sum(1)[:, None] - 2.0 * z @ e.T + (e ** 2).sum(1)[None]
    ar = np.arange(rows)
    # exact copies of a code row are one code: k* is the lowest index of the best row's copies, and
    # the margin runs to the best row that differs from it
    first_copy = np.asarray([int(np.flatnonzero((e == e[k]).all(1))[0]) for k in range(e.shape[0])])
    kstar = first_copy[np.argmin(d, axis=1)]
    others = np.where(first_copy[None, :] == kstar[:, None], np.inf, d)
    second = np.argmin(others, axis=1)
    margin = others[ar, second] - d[ar, kstar]
    tau = 2.0 * (D + 2) * U * (np.linalg.norm(z, axis=1) + np.linalg.norm(e, axis=1).max()) ** 2
    allow = tau.copy()
    allow_margin = tau.copy()
    if z_used is not None:
        delta = np.linalg.norm(np.asarray(z_used, np.float64) - z, axis=1)
        allow = tau + 2.0 * delta * np.linalg.norm(e[idx] - e[kstar], axis=1)
        allow_margin = tau + 2.0 * delta * np.linalg.norm(e[second] - e[kstar], axis=1)
    gap = d[ar, idx] - d[ar, kstar]
    violations = int((gap > allow).sum())
    under = margin <= allow_margin
    mismatches = 0
    if ref_idx is not None:
        ref_idx = np.asarray(ref_idx).astype(np.int64).reshape(-1)
        mismatches = int(((idx != ref_idx) & ~under).sum())
    return violations, int(under.sum()), mismatches


def cap(rows):
    """At most 2 % of the frames may fall under their allowance, one frame always permitted."""
    return max(1, int(0.02 * rows))
