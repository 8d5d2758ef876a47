"""Torch restatement of the StyleMelGAN generator, written from its formulas, for
the tests that cannot use fixtures (ragged batches, block-wise comparison) and as the eager baseline
of tools/stylemelgan_bench.py. float64 on the CPU by default.

Per utterance, with C = channels, K = kernel_size, d = dilation:
  x  = noise upsampling of z: per scale s ConvTranspose1d(kernel 2 s, stride s, padding s//2 + s%2,
       output_padding s%2) + LeakyReLU; N0 = Lz * prod(scales) rows
  c  = the T aux frames (optionally (c - mean) / scale), replicate-padded on the right to N0
  per block with scale s:   IN(v) = (v - mean_t) * rsqrt(var_t + 1e-5) (biased), up_s(a)[t] = a[t // s]
      c1 = aux_conv1(c);  cg = gated_conv(c1);  y = cg[:C] * IN(x) + cg[C:]
      g = gated_conv1(y);  x1 = gate(g[:C]) * tanh(g[C:])
      c2 = aux_conv2(up_s(c1));  cg = gated_conv(c2);  y = cg[:C] * up_s(IN(x1)) + cg[C:]
      g = gated_conv2(y) (dilation d);  x = up_s(x) + gate(g[:C]) * tanh(g[C:]);  c = c2
  out = tanh(output_conv(x))[: T * prod(upsample_scales)]
Every conv is zero-padded "same". Tensors here are (channels, time).
"""

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5


class Oracle:
    def __init__(self, folded, params, dtype=torch.float64, device="cpu"):
        """folded: state dict with weight norm folded ({key: ndarray})."""
        self.p = params
        self.dtype, self.device = dtype, device
        self.w = {k: torch.as_tensor(np.asarray(v), dtype=dtype, device=device) for k, v in folded.items()
                  if k not in ("mean", "scale")}
        self.noise_factor = int(np.prod(params["noise_upsample_scales"]))
        self.hop = int(np.prod(params["upsample_scales"]))

    def _conv(self, x, name, dilation=1):
        w = self.w[name + ".weight"]
        return F.conv1d(x[None], w, self.w.get(name + ".bias"), padding=(w.shape[2] - 1) // 2 * dilation,
                        dilation=dilation)[0]

    @staticmethod
    def _in(x):
        mean = x.mean(1, keepdim=True)
        var = ((x - mean) ** 2).mean(1, keepdim=True)
        return (x - mean) * torch.rsqrt(var + EPS), mean[:, 0], torch.rsqrt(var + EPS)[:, 0]

    def _gate(self, g):
        C = g.shape[0] // 2
        a = torch.softmax(g[:C], 0) if self.p.get("gated_function", "softmax") == "softmax" else torch.sigmoid(g[:C])
        return a * torch.tanh(g[C:])

    def noise_upsample(self, z):
        x = z
        slope = self.p.get("noise_upsample_activation_params", {}).get("negative_slope", 0.01)
        for i, s in enumerate(self.p["noise_upsample_scales"]):
            n = f"noise_upsample.{2 * i}"
            x = F.conv_transpose1d(x[None], self.w[n + ".weight"], self.w.get(n + ".bias"), stride=s,
                                   padding=s // 2 + s % 2, output_padding=s % 2)[0]
            x = F.leaky_relu(x, slope)
        return x

    def __call__(self, c, z, mean=None, scale=None, blocks=None):
        """c (T, aux), z (Lz, in_channels) -> (T * hop, out_channels). blocks: a list that receives
        per block a dict(x_in, x_out (channels, rows), stats_in, stats_mid ((mean, rstd) each))."""
        c = torch.as_tensor(np.asarray(c) if not torch.is_tensor(c) else c).to(self.device, self.dtype)
        z = torch.as_tensor(np.asarray(z) if not torch.is_tensor(z) else z).to(self.device, self.dtype)
        T = c.shape[0]
        if mean is not None:
            c = (c - torch.as_tensor(mean).to(self.device, self.dtype)) / torch.as_tensor(scale).to(self.device, self.dtype)
        x = self.noise_upsample(z.T)
        c = c.T
        assert x.shape[1] >= T
        c = torch.cat([c, c[:, -1:].expand(-1, x.shape[1] - T)], 1)
        for i, s in enumerate(self.p["upsample_scales"]):
            b = f"blocks.{i}."
            C = x.shape[0]
            xn, m0, r0 = self._in(x)
            c1 = self._conv(c, b + "tade1.aux_conv.0")
            cg = self._conv(c1, b + "tade1.gated_conv.0")
            y = cg[:C] * xn + cg[C:]
            x1 = self._gate(self._conv(y, b + "gated_conv1"))
            x1n, m1, r1 = self._in(x1)
            c2 = self._conv(c1.repeat_interleave(s, 1), b + "tade2.aux_conv.0")
            cg = self._conv(c2, b + "tade2.gated_conv.0")
            y = cg[:C] * x1n.repeat_interleave(s, 1) + cg[C:]
            xo = x.repeat_interleave(s, 1) + self._gate(self._conv(y, b + "gated_conv2", self.p["dilation"]))
            if blocks is not None:
                blocks.append(dict(x_in=x, x_out=xo, stats_in=(m0, r0), stats_mid=(m1, r1)))
            x, c = xo, c2
        y = torch.tanh(self._conv(x, "output_conv.0"))[:, : T * self.hop]
        return y.T
