"""Torch restatement of DiscreteSymbolStyleMelGANGenerator on top of the block
oracle of tests/stylemelgan_oracle.py, which is imported unchanged: the token front end
  c[t] = emb[ids[t]] + spk_emb[g]        (g: the speaker id of the utterance's first frame, or given)
and the trim x = noise_upsample(z)[:, :T] in place of the replicate padding of c. With T rows of x the
base oracle pads c by nothing, so its blocks, statistics and output conv run over exactly T rows per
utterance. float64 on the CPU by default; tools/dsym_stylemelgan_bench.py runs it in fp32 on the GPU as
the eager baseline.
"""

import numpy as np
import torch

from stylemelgan_oracle import Oracle


class TokenOracle(Oracle):
    _trim = None

    def noise_upsample(self, z):
        x = super().noise_upsample(z)
        return x if self._trim is None else x[:, : self._trim]

    def embed(self, ids, g=None):
        """ids (T, 2), or (T, 1) / (T,) with g -> c (T, aux)."""
        ids = torch.as_tensor(np.asarray(ids) if not torch.is_tensor(ids) else ids).long().to(self.device)
        tok = ids if ids.dim() == 1 else ids[:, 0]
        spk = int(ids[0, 1]) if g is None else int(g)
        return self.w["emb.weight"][tok] + self.w["spk_emb.weight"][spk]

    def __call__(self, ids, z, g=None, blocks=None):
        """ids (T, 2), z (Lz, in_channels) -> (T * hop, out_channels); blocks as in the base class."""
        c = self.embed(ids, g)
        self._trim = c.shape[0]
        try:
            return super().__call__(c, z, blocks=blocks)
        finally:
            self._trim = None
