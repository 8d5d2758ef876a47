"""Generator configurations of the benchmark recipes (``generator_params`` blocks).

Values are restated from the reference recipe YAMLs:
  yesno_debug  egs/yesno/voc1/conf/parallel_wavegan.v1.debug.yaml:26-44 (fs 8 kHz, hop 256)
  ljspeech_v1  egs/ljspeech/voc1/conf/parallel_wavegan.v1.yaml:28-46   (fs 22.05 kHz, hop 256)
  libritts_v1  egs/libritts/voc1/conf/parallel_wavegan.v1.yaml:28-46   (fs 24 kHz, hop 300)
``reference_test`` is the small generator of the reference unit tests
(test/test_parallel_wavegan.py:31-51) with dropout removed.
"""

import copy

_PWG_V1 = dict(
    in_channels=1,
    out_channels=1,
    kernel_size=3,
    layers=30,
    stacks=3,
    residual_channels=64,
    gate_channels=128,
    skip_channels=64,
    aux_channels=80,
    aux_context_window=2,
    dropout=0.0,
    use_weight_norm=True,
    upsample_net="ConvInUpsampleNetwork",
    upsample_params={"upsample_scales": [4, 4, 4, 4]},
)

GENERATOR_PARAMS = {
    "yesno_debug": dict(
        _PWG_V1,
        layers=20,
        stacks=2,
        residual_channels=16,
        gate_channels=32,
        skip_channels=16,
        aux_context_window=1,
    ),
    "ljspeech_v1": dict(_PWG_V1),
    "libritts_v1": dict(_PWG_V1, upsample_params={"upsample_scales": [4, 5, 3, 5]}),
    "reference_test": dict(
        in_channels=1,
        out_channels=1,
        kernel_size=3,
        layers=6,
        stacks=3,
        residual_channels=8,
        gate_channels=16,
        skip_channels=8,
        aux_channels=10,
        aux_context_window=2,
        dropout=0.0,
        use_weight_norm=True,
        use_causal_conv=False,
        upsample_conditional_features=True,
        upsample_net="ConvInUpsampleNetwork",
        upsample_params={"upsample_scales": [4, 4]},
    ),
}

SAMPLING_RATE = {
    "yesno_debug": 8000,
    "ljspeech_v1": 22050,
    "libritts_v1": 24000,
    "reference_test": 16000,
}


def generator_params(name, **overrides):
    """Deep copy of a recipe's generator_params (the constructor mutates upsample_params,
    models/parallel_wavegan.py:85-107, so callers must never share the dict)."""
    p = copy.deepcopy(GENERATOR_PARAMS[name])
    p.update(copy.deepcopy(overrides))
    return p


# MelGAN-family generators, executed by the conv-network engine.
#   melgan_v1     egs/ljspeech/voc1/conf/melgan.v1.yaml (generator_params)
#   mb_melgan_v2  egs/ljspeech/voc1/conf/multi_band_melgan.v2.yaml:38-48, + PQMF(4) synthesis
#   hifigan_v1    egs/ljspeech/voc1/conf/hifigan.v1.yaml:32-50
# ``*_test`` are reduced shapes for parity fixtures (same code paths, seconds on the oracle).
VOCODER_PARAMS = {
    "melgan_v1": ("MelGANGenerator", dict(in_channels=80, out_channels=1, kernel_size=7, channels=512,
                                          upsample_scales=[8, 8, 2, 2], stack_kernel_size=3, stacks=3,
                                          use_weight_norm=True, use_causal_conv=False)),
    "mb_melgan_v2": ("MelGANGenerator", dict(in_channels=80, out_channels=4, kernel_size=7, channels=384,
                                             upsample_scales=[8, 4, 2], stack_kernel_size=3, stacks=4,
                                             use_weight_norm=True, use_causal_conv=False)),
    "hifigan_v1": ("HiFiGANGenerator", dict(in_channels=80, out_channels=1, channels=512, kernel_size=7,
                                            upsample_scales=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4],
                                            resblock_kernel_sizes=[3, 7, 11],
                                            resblock_dilations=[[1, 3, 5], [1, 3, 5], [1, 3, 5]],
                                            use_additional_convs=True, bias=True,
                                            nonlinear_activation="LeakyReLU",
                                            nonlinear_activation_params={"negative_slope": 0.1},
                                            use_weight_norm=True)),
    "mb_melgan_test": ("MelGANGenerator", dict(in_channels=80, out_channels=4, kernel_size=7, channels=64,
                                               upsample_scales=[4, 2], stack_kernel_size=3, stacks=3,
                                               use_weight_norm=True, use_causal_conv=False)),
    "melgan_test": ("MelGANGenerator", dict(in_channels=80, out_channels=1, kernel_size=7, channels=96,
                                            upsample_scales=[3, 2, 2], stack_kernel_size=3, stacks=2,
                                            use_weight_norm=True, use_causal_conv=False)),
    "hifigan_test": ("HiFiGANGenerator", dict(in_channels=80, out_channels=1, channels=64, kernel_size=7,
                                              upsample_scales=[4, 2], upsample_kernel_sizes=[8, 4],
                                              resblock_kernel_sizes=[3, 5], resblock_dilations=[[1, 3], [1, 2]],
                                              use_additional_convs=True, bias=True,
                                              nonlinear_activation="LeakyReLU",
                                              nonlinear_activation_params={"negative_slope": 0.1},
                                              use_weight_norm=True)),
    "hifigan_noadd_test": ("HiFiGANGenerator", dict(in_channels=80, out_channels=1, channels=32, kernel_size=5,
                                                    upsample_scales=[3], upsample_kernel_sizes=[6],
                                                    resblock_kernel_sizes=[3, 5, 7],
                                                    resblock_dilations=[[1, 3], [1, 2], [2, 1]],
                                                    use_additional_convs=False, bias=True,
                                                    nonlinear_activation="LeakyReLU",
                                                    nonlinear_activation_params={"negative_slope": 0.1},
                                                    use_weight_norm=True)),
}

def _causal(name, **over):
    cls, p = VOCODER_PARAMS[name]
    p = copy.deepcopy(p)
    p.update(use_causal_conv=True, **over)
    return cls, p


# causal variants (models/melgan.py:73-151, models/hifigan.py:83-164, layers/causal_conv.py;
# the reference's causality tests use odd and mixed upsample scales, test/test_hifigan.py:163-196,
# test/test_melgan.py:267-274)
VOCODER_PARAMS.update({
    "melgan_causal_test": _causal("melgan_test"),
    "mb_melgan_causal_test": _causal("mb_melgan_test", upsample_scales=[3, 2]),
    "hifigan_causal_test": _causal("hifigan_test", upsample_scales=[5, 3], upsample_kernel_sizes=[10, 6]),
    "hifigan_noadd_causal_test": _causal("hifigan_noadd_test"),
    "mb_melgan_v2_causal": _causal("mb_melgan_v2"),
    "hifigan_v1_causal": _causal("hifigan_v1"),
    "melgan_v1_causal": _causal("melgan_v1"),
})
VOCODER_PQMF = {"mb_melgan_v2": dict(subbands=4), "mb_melgan_test": dict(subbands=4),
                "mb_melgan_v2_causal": dict(subbands=4), "mb_melgan_causal_test": dict(subbands=4)}
SAMPLING_RATE.update(melgan_v1=22050, mb_melgan_v2=22050, hifigan_v1=22050)

# Discrete-symbol (token) HiFiGAN vocoders (models/hifigan.py:867-1097): ids in, HiFiGAN v1 body.
#   dsym_hubert_v1  egs/vctk/hubert_voc1/conf/hifigan_hubert.v1.yaml:26-48 (16 kHz, hop 320)
#   dsym_token_v1   egs/opencpop/token_voc1/conf/hifigan_token_16k_nodp.v1.yaml:28-48 (no speaker table)
# ``*_test`` are reduced shapes: with a speaker table, without one, and fed features directly.
_DSYM_V1 = dict(out_channels=1, channels=512, concat_spk_emb=False, kernel_size=7, upsample_scales=[10, 8, 2, 2],
                upsample_kernel_sizes=[20, 16, 4, 4], resblock_kernel_sizes=[3, 7, 11],
                resblock_dilations=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], use_additional_convs=True, bias=True,
                nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1},
                use_weight_norm=True)
_DSYM_TEST = dict(in_channels=48, out_channels=1, channels=64, num_embs=11, num_spk_embs=5, spk_emb_dim=48,
                  concat_spk_emb=False, kernel_size=7, upsample_scales=[4, 2], upsample_kernel_sizes=[8, 4],
                  resblock_kernel_sizes=[3, 5], resblock_dilations=[[1, 3], [1, 2]], use_additional_convs=True,
                  bias=True, nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1},
                  use_weight_norm=True)
VOCODER_PARAMS.update({
    "dsym_hifigan_test": ("DiscreteSymbolHiFiGANGenerator", dict(_DSYM_TEST)),
    "dsym_hifigan_nospk_test": ("DiscreteSymbolHiFiGANGenerator", dict(_DSYM_TEST, num_spk_embs=0)),
    "dsym_hifigan_feats_test": ("DiscreteSymbolHiFiGANGenerator",
                                dict(_DSYM_TEST, num_spk_embs=0, use_embedding_feats=True)),
    "dsym_hubert_v1": ("DiscreteSymbolHiFiGANGenerator",
                       dict(_DSYM_V1, in_channels=512, num_embs=100, num_spk_embs=128, spk_emb_dim=512)),
    "dsym_token_v1": ("DiscreteSymbolHiFiGANGenerator",
                      dict(_DSYM_V1, in_channels=768, num_embs=1025, num_spk_embs=0)),
})
SAMPLING_RATE.update(dsym_hubert_v1=16000, dsym_token_v1=16000)

# Duration- and f0-conditioned token vocoders (models/hifigan.py:1100-1487; dsym_variants.py).
#   dsym_duration_v1         egs/cvss_c/hubert_voc1/conf/hifigan_hubert_duration.v1.yaml (predictor 512 -> 384)
#   dsym_token_duration_16k  egs/opencpop/token_voc1/conf/hifigan_token_16k_duration.v1.yaml (1024 -> 384)
#   dsym_f0_v1               egs/opencpop/token_voc1/conf/hifigan_token_16k_nodp_f0.v1.yaml (768 + 256)
# ``*_test`` are reduced shapes on _DSYM_TEST.
_DSYM_DUR = dict(num_spk_embs=0, duration_layers=2, duration_chans=384, duration_kernel_size=3, duration_offset=1.0,
                 duration_dropout_rate=0.5)
VOCODER_PARAMS.update({
    "dsym_duration_test": ("DiscreteSymbolDurationGenerator",
                           dict(_DSYM_TEST, num_spk_embs=0, duration_chans=32, duration_layers=2)),
    "dsym_f0_test": ("DiscreteSymbolF0Generator", dict(_DSYM_TEST, num_spk_embs=0, linear_channel=16)),
    "dsym_f0_spk_test": ("DiscreteSymbolF0Generator", dict(_DSYM_TEST, linear_channel=16)),
    "dsym_f0_wsum_test": ("DiscreteSymbolF0Generator",
                          dict(_DSYM_TEST, num_spk_embs=0, linear_channel=16, use_weight_sum=True, layer_num=3)),
    "dsym_f0_wsum_fix_test": ("DiscreteSymbolF0Generator",
                              dict(_DSYM_TEST, num_spk_embs=0, linear_channel=16, use_weight_sum=True, layer_num=3,
                                   use_fix_weight=True)),
    "dsym_duration_v1": ("DiscreteSymbolDurationGenerator",
                         dict(_DSYM_V1, **_DSYM_DUR, in_channels=512, num_embs=500, spk_emb_dim=512)),
    "dsym_token_duration_16k": ("DiscreteSymbolDurationGenerator",
                                dict(_DSYM_V1, **_DSYM_DUR, in_channels=1024, num_embs=1024, spk_emb_dim=512)),
    "dsym_f0_v1": ("DiscreteSymbolF0Generator",
                   dict(_DSYM_V1, in_channels=768, linear_channel=256, num_embs=1025, num_spk_embs=0)),
})
SAMPLING_RATE.update(dsym_duration_v1=16000, dsym_token_duration_16k=16000, dsym_f0_v1=16000)


def vocoder_params(name, **overrides):
    """(generator class name, deep-copied generator_params) of a MelGAN-family recipe."""
    cls, p = VOCODER_PARAMS[name]
    p = copy.deepcopy(p)
    p.update(copy.deepcopy(overrides))
    return cls, p


# StyleMelGAN generators (models/style_melgan.py:18-240), a table of their own: they run on the
# TADE kernels (include/pwg_smg.h), not on the conv-network executor.
#   style_melgan_v1  egs/{ljspeech,libritts,vctk,jsut,csmsc,yesno}/voc1/conf/style_melgan.v1*.yaml
# ``*_test`` are reduced shapes: the softmax gate with even scales, and a sigmoid gate with odd
# noise and upsample scales, with and without biases.
STYLE_MELGAN_PARAMS = {
    "style_melgan_v1": dict(in_channels=128, aux_channels=80, channels=64, out_channels=1, kernel_size=9, dilation=2,
                            bias=True, noise_upsample_scales=[11, 2, 2, 2], noise_upsample_activation="LeakyReLU",
                            noise_upsample_activation_params={"negative_slope": 0.2},
                            upsample_scales=[2, 2, 2, 2, 2, 2, 2, 2, 1], upsample_mode="nearest",
                            gated_function="softmax", use_weight_norm=True),
    "style_melgan_test": dict(in_channels=32, aux_channels=80, channels=64, out_channels=1, kernel_size=9, dilation=2,
                              bias=True, noise_upsample_scales=[4, 2], noise_upsample_activation="LeakyReLU",
                              noise_upsample_activation_params={"negative_slope": 0.2},
                              upsample_scales=[2, 2, 2, 1], upsample_mode="nearest", gated_function="softmax",
                              use_weight_norm=True),
    "style_melgan_odd_test": dict(in_channels=32, aux_channels=16, channels=32, out_channels=1, kernel_size=5,
                                  dilation=2, bias=True, noise_upsample_scales=[3, 2],
                                  noise_upsample_activation="LeakyReLU",
                                  noise_upsample_activation_params={"negative_slope": 0.2},
                                  upsample_scales=[3, 1, 2], upsample_mode="nearest", gated_function="sigmoid",
                                  use_weight_norm=True),
}
STYLE_MELGAN_PARAMS["style_melgan_odd_nobias_test"] = dict(STYLE_MELGAN_PARAMS["style_melgan_odd_test"], bias=False)


def style_melgan_params(name, **overrides):
    """Deep-copied StyleMelGANGenerator constructor arguments of a recipe."""
    p = copy.deepcopy(STYLE_MELGAN_PARAMS[name])
    p.update(copy.deepcopy(overrides))
    return p


# Token StyleMelGAN generators (DiscreteSymbolStyleMelGANGenerator, models/style_melgan.py:364-602;
# dsym_stylemelgan.py): ids and a speaker id in, the TADE kernels with the token staging and the
# trimmed layout (include/pwg_smg.h).
#   dsym_style_melgan_hubert_v1  egs/vctk/hubert_voc1/conf/style_melgan_hubert.v1.yaml:25-45 (16 kHz, hop 320:
#                                an odd noise scale, a factor-5 block and two factor-1 blocks)
# ``*_test`` are reduced shapes: the softmax gate at aux 128, and a sigmoid gate with odd scales, with and
# without biases.
DSYM_STYLE_MELGAN_PARAMS = {
    "dsym_style_melgan_hubert_v1": dict(in_channels=128, aux_channels=128, channels=64, out_channels=1, num_embs=100,
                                        num_spk_embs=128, spk_emb_dim=128, concat_spk_emb=False, kernel_size=9,
                                        dilation=2, bias=True, noise_upsample_scales=[7, 2, 2, 2],
                                        noise_upsample_activation="LeakyReLU",
                                        noise_upsample_activation_params={"negative_slope": 0.2},
                                        upsample_scales=[5, 2, 2, 2, 2, 2, 2, 1, 1], upsample_mode="nearest",
                                        gated_function="softmax", use_weight_norm=True),
    "dsym_smg_test": dict(in_channels=32, aux_channels=128, channels=64, out_channels=1, num_embs=11, num_spk_embs=3,
                          spk_emb_dim=128, concat_spk_emb=False, kernel_size=9, dilation=2, bias=True,
                          noise_upsample_scales=[4, 2], noise_upsample_activation="LeakyReLU",
                          noise_upsample_activation_params={"negative_slope": 0.2}, upsample_scales=[2, 2, 2, 1],
                          upsample_mode="nearest", gated_function="softmax", use_weight_norm=True),
    "dsym_smg_odd_test": dict(in_channels=32, aux_channels=32, channels=32, out_channels=1, num_embs=11,
                              num_spk_embs=3, spk_emb_dim=32, concat_spk_emb=False, kernel_size=5, dilation=2,
                              bias=True, noise_upsample_scales=[3, 2], noise_upsample_activation="LeakyReLU",
                              noise_upsample_activation_params={"negative_slope": 0.2}, upsample_scales=[3, 1, 2],
                              upsample_mode="nearest", gated_function="sigmoid", use_weight_norm=True),
}
DSYM_STYLE_MELGAN_PARAMS["dsym_smg_odd_nobias_test"] = dict(DSYM_STYLE_MELGAN_PARAMS["dsym_smg_odd_test"], bias=False)
SAMPLING_RATE.update(dsym_style_melgan_hubert_v1=16000)


def dsym_style_melgan_params(name, **overrides):
    """Deep-copied DiscreteSymbolStyleMelGANGenerator constructor arguments of a recipe."""
    p = copy.deepcopy(DSYM_STYLE_MELGAN_PARAMS[name])
    p.update(copy.deepcopy(overrides))
    return p


# UHiFiGAN generators (models/uhifigan.py:19-387), a table of their own: they take an excitation
# signal besides the mel, and the MelGAN-family tests iterate VOCODER_PARAMS.
#   uhifigan_v1  egs/{opencpop,opensinger}/voc1/conf/uhifigan.v1.yaml (24 kHz singing, hop 300)
# ``*_test`` are reduced shapes: odd and even scales with two residual-block shapes, and a variant
# without additional convs or biases.
UHIFIGAN_PARAMS = {
    "uhifigan_v1": dict(in_channels=80, out_channels=1, channels=32, kernel_size=7,
                        downsample_scales=[5, 5, 4, 3], downsample_kernel_sizes=[10, 10, 8, 6],
                        upsample_scales=[3, 4, 5, 5], upsample_kernel_sizes=[6, 8, 10, 10],
                        resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5], [1, 3, 5], [1, 3, 5]],
                        dropout=0.1, use_additional_convs=True, bias=True, nonlinear_activation="LeakyReLU",
                        nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True),
    "uhifigan_test": dict(in_channels=80, out_channels=1, channels=32, kernel_size=7,
                          downsample_scales=[3, 2, 2], downsample_kernel_sizes=[6, 4, 4],
                          upsample_scales=[2, 2, 3], upsample_kernel_sizes=[4, 4, 6],
                          resblock_kernel_sizes=[3, 5], resblock_dilations=[[1, 3], [1, 2]],
                          dropout=0.1, use_additional_convs=True, bias=True, nonlinear_activation="LeakyReLU",
                          nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True),
    "uhifigan_noadd_nobias_test": dict(in_channels=16, out_channels=1, channels=32, kernel_size=5,
                                       downsample_scales=[5, 4], downsample_kernel_sizes=[10, 8],
                                       upsample_scales=[4, 5], upsample_kernel_sizes=[8, 10],
                                       resblock_kernel_sizes=[3], resblock_dilations=[[1, 2]],
                                       dropout=0.1, use_additional_convs=False, bias=False,
                                       nonlinear_activation="LeakyReLU",
                                       nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True),
}


def uhifigan_params(name, **overrides):
    """Deep-copied UHiFiGANGenerator constructor arguments of a recipe."""
    p = copy.deepcopy(UHIFIGAN_PARAMS[name])
    p.update(copy.deepcopy(overrides))
    return p


# VQVAE (models/vqvae.py:16-171), a table of its own: waveform in, codes and waveform out.
#   vqvae_v3  egs/vctk/vq1/conf/local_conditioned_melgan_vae.v3.yaml (24 kHz, hop 64, local 2 -> 32,
#             global 128 x 128, decoder in_channels 416); without the local part the decoder takes 384
#             channels, without both 256 (overrides).
# ``*_test`` are reduced shapes: ``a`` has a level of 16 outputs per group and one of 4 (the width
# cap), 48 codes and both conditionings; ``b`` two levels of 8 outputs per group, 33 codes, no
# conditioning and no encoder biases.
VQVAE_PARAMS = {
    "vqvae_v3": dict(in_channels=1, out_channels=1, num_embeds=512, embed_dim=256, num_local_embeds=2,
                     local_embed_dim=32, num_global_embeds=128, global_embed_dim=128,
                     encoder_type="MelGANDiscriminator", decoder_type="MelGANGenerator",
                     encoder_conf=dict(out_channels=256, downsample_scales=[4, 4, 2, 2], max_downsample_channels=1024),
                     decoder_conf=dict(in_channels=416, upsample_scales=[4, 4, 2, 2], channels=512, stacks=3),
                     use_weight_norm=True),
    "vqvae_test_a": dict(in_channels=1, out_channels=1, num_embeds=48, embed_dim=32, num_local_embeds=2,
                         local_embed_dim=16, num_global_embeds=5, global_embed_dim=16,
                         encoder_type="MelGANDiscriminator", decoder_type="MelGANGenerator",
                         encoder_conf=dict(channels=16, downsample_scales=[4, 2], max_downsample_channels=64,
                                           out_channels=32),
                         decoder_conf=dict(in_channels=64, channels=64, upsample_scales=[4, 2], stacks=2),
                         use_weight_norm=True),
    "vqvae_test_b": dict(in_channels=1, out_channels=1, num_embeds=33, embed_dim=32,
                         encoder_type="MelGANDiscriminator", decoder_type="MelGANGenerator",
                         encoder_conf=dict(channels=16, downsample_scales=[2, 2], max_downsample_channels=64,
                                           out_channels=32, bias=False),
                         decoder_conf=dict(in_channels=32, channels=64, upsample_scales=[2, 2], stacks=2),
                         use_weight_norm=True),
}
SAMPLING_RATE.update(vqvae_v3=24000)


def vqvae_params(name, **overrides):
    """Deep-copied VQVAE constructor arguments of a recipe."""
    p = copy.deepcopy(VQVAE_PARAMS[name])
    p.update(copy.deepcopy(overrides))
    return p
