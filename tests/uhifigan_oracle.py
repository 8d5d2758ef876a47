"""Float64 torch restatement of the UHiFiGAN generator (eval semantics) for the GPU tests: written
from the network's definition for this project, it takes a folded state dict (no weight norm) and can
return every intermediate tensor the executor keeps in a buffer. Not a test module.

    h = lrelu(conv(excitation))                                  input_conv
    per level i:  h = mean_j block_j(h);  h = lrelu(strided_conv(h));  skip_i = h
    g = conv(mel)                                                hidden_conv
    per level i:  g = convT(lrelu(cat(g, skip_{n-1-i})));  g = mean_j block_j(g)
    y = tanh(conv(lrelu_0.01(g)))

A residual block is x <- x + conv2(lrelu(conv1(lrelu(x)))) per dilation (conv2 with dilation 1 and
only with additional convs).
"""

import torch
import torch.nn.functional as F


class Oracle:
    def __init__(self, folded, params):
        self.w = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in folded.items()}
        self.p = params
        self.slope = float(params["nonlinear_activation_params"]["negative_slope"])
        self.nb = len(params["resblock_kernel_sizes"])

    def _conv(self, key, x, **kw):
        return F.conv1d(x, self.w[key + ".weight"], self.w.get(key + ".bias"), **kw)

    def _block(self, key, j, x):
        k = self.p["resblock_kernel_sizes"][j]
        for d, dil in enumerate(self.p["resblock_dilations"][j]):
            t = self._conv(f"{key}.convs1.{d}.1", F.leaky_relu(x, self.slope), dilation=dil, padding=(k - 1) // 2 * dil)
            if self.p["use_additional_convs"]:
                t = self._conv(f"{key}.convs2.{d}.1", F.leaky_relu(t, self.slope), padding=(k - 1) // 2)
            x = x + t
        return x

    def _mrf(self, prefix, i, x):
        cs = 0.0
        for j in range(self.nb):
            cs = cs + self._block(f"{prefix}.{i * self.nb + j}", j, x)
        return cs / self.nb

    def __call__(self, c, excitation, levels=None):
        """c (T, in_channels), excitation (T * hop,) -> (T * hop, 1) float64. ``levels`` (a dict)
        receives the intermediate tensors, each (rows, channels): excite, down_mrf[i], down[i],
        hidden, up[i], up_mrf[i]."""
        p = self.p
        pad = (p["kernel_size"] - 1) // 2
        c = torch.as_tensor(c, dtype=torch.float64).T.unsqueeze(0)
        e = torch.as_tensor(excitation, dtype=torch.float64).reshape(1, 1, -1)
        keep = dict(down_mrf=[], down=[], up=[], up_mrf=[])
        h = F.leaky_relu(self._conv("input_conv.0", e, padding=pad), self.slope)
        keep["excite"] = h
        skips = []
        for i, s in enumerate(p["downsample_scales"]):
            h = self._mrf("downsamples_mrf", i, h)
            keep["down_mrf"].append(h)
            h = F.leaky_relu(self._conv(f"downsamples.{i}.0", h, stride=s, padding=s // 2 + s % 2), self.slope)
            keep["down"].append(h)
            skips.append(h)
        g = self._conv("hidden_conv", c, padding=pad)
        keep["hidden"] = g
        for i, s in enumerate(p["upsample_scales"]):
            g = torch.cat((g, skips[len(skips) - 1 - i]), dim=1)
            g = F.conv_transpose1d(F.leaky_relu(g, self.slope), self.w[f"upsamples.{i}.1.weight"],
                                   self.w.get(f"upsamples.{i}.1.bias"), stride=s, padding=s // 2 + s % 2,
                                   output_padding=s % 2)
            keep["up"].append(g)
            g = self._mrf("upsamples_mrf", i, g)
            keep["up_mrf"].append(g)
        y = torch.tanh(self._conv("output_conv.1", F.leaky_relu(g, 0.01), padding=pad))
        if levels is not None:
            for k, v in keep.items():
                levels[k] = [t[0].T for t in v] if isinstance(v, list) else v[0].T
        return y[0].T
