"""CPU: the tables PretrainEngine derives from its declarations -- the flat layout, the per-layer slab ranges, the head /
pooler ranges that go to the communicator first, the shard atoms and launch ranges, the fp32 spans, the mirror-only
names and the transpose batch -- pinned to literal values for a two-layer model and three variants of it; and the shape
of the step state (one declared class, shared by the bf16 and the fp32 step)."""
import ast
import os

import pytest
import torch

from visitron_amd import ops, training, training_f32
from visitron_amd.config import BertConfig
from visitron_amd.modeling import PreTrainOscar
from visitron_amd.training import PretrainEngine

VARIANTS = ("plain", "img_layernorm", "untied", "trunk")


def _engine(variant):
    cfg = BertConfig(vocab_size=97, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=32, img_feature_dim=20, detector_classes=11, action_space=5)
    if variant == "img_layernorm":
        cfg.use_img_layernorm, cfg.img_layer_norm_eps = 1, 1e-12
    torch.manual_seed(0)
    m = PreTrainOscar(cfg)
    if variant == "untied":
        m.resize_embeddings({"word_embeddings": cfg.vocab_size + 3})
    return PretrainEngine(m.bert if variant == "trunk" else m)


class _RecordedBatch(object):
    """Stands in for ops.TransposeBatch on the host: keeps the pairs, launches nothing."""
    pairs = None

    def __init__(self, pairs):
        _RecordedBatch.pairs = list(pairs)

    def run(self):
        pass


def _describe(eng, monkeypatch):
    f = eng.flat
    monkeypatch.setattr(ops, "TransposeBatch", _RecordedBatch)
    eng.refresh_derived_weights()
    at = {o: n for n, (o, _, _) in f.off.items()}
    transposes = [(at[(s.data_ptr() - f.mirror.data_ptr()) // 2], tuple(s.shape), tuple(d.shape)) for s, d in _RecordedBatch.pairs]
    # ... and which transposed head copy each pair writes (None: a layer's own)
    head_dst = [next((k for k, v in eng.head_t.items() if v.data_ptr() == d.data_ptr()), None) for _, d in _RecordedBatch.pairs]
    return dict(total=f.total, n_decay=f.n_decay, off=dict(f.off), layer_ranges=eng.layer_ranges,
                head_ranges=eng._param_ranges(eng._head_params()) if eng.has_heads else None,
                shard_atoms=eng.shard_atoms(), shard_launch_ranges=eng.shard_launch_ranges(), fp32_spans=eng.fp32_spans(),
                mirror_only=sorted(eng.mirror_only_names()), transposes=transposes, head_dst=head_dst)


# recorded from the engine as it stood before its tables were declared once (same statements as _describe)
EXPECTED = {'plain': {'total': 336768,
           'n_decay': 332672,
           'off': {'bert.embeddings.word_embeddings.weight': (0, 12416, (97, 128)),
                   'bert.embeddings.position_embeddings.weight': (12416, 4096, (32, 128)),
                   'bert.embeddings.token_type_embeddings.weight': (16512, 256, (2, 128)),
                   'bert.encoder.layer.0.attention.self.query.weight': (16768, 16384, (128, 128)),
                   'bert.encoder.layer.0.attention.self.key.weight': (33152, 16384, (128, 128)),
                   'bert.encoder.layer.0.attention.self.value.weight': (49536, 16384, (128, 128)),
                   'bert.encoder.layer.0.attention.output.dense.weight': (65920, 16384, (128, 128)),
                   'bert.encoder.layer.0.intermediate.dense.weight': (82304, 32768, (256, 128)),
                   'bert.encoder.layer.0.output.dense.weight': (115072, 32768, (128, 256)),
                   'bert.encoder.layer.1.attention.self.query.weight': (147840, 16384, (128, 128)),
                   'bert.encoder.layer.1.attention.self.key.weight': (164224, 16384, (128, 128)),
                   'bert.encoder.layer.1.attention.self.value.weight': (180608, 16384, (128, 128)),
                   'bert.encoder.layer.1.attention.output.dense.weight': (196992, 16384, (128, 128)),
                   'bert.encoder.layer.1.intermediate.dense.weight': (213376, 32768, (256, 128)),
                   'bert.encoder.layer.1.output.dense.weight': (246144, 32768, (128, 256)),
                   'bert.pooler.dense.weight': (278912, 16384, (128, 128)),
                   'bert.img_embedding.weight': (295296, 2560, (128, 20)),
                   'bert.location_embeds.weight': (297856, 16384, (128, 128)),
                   'next_action.linear.weight': (314240, 640, (5, 128)),
                   'mlmhead.predictions.transform.dense.weight': (314880, 16384, (128, 128)),
                   'token_head.0.weight': (331264, 1408, (11, 128)),
                   'bert.embeddings.LayerNorm.weight': (332672, 128, (128,)),
                   'bert.embeddings.LayerNorm.bias': (332800, 128, (128,)),
                   'bert.encoder.layer.0.attention.self.query.bias': (332928, 128, (128,)),
                   'bert.encoder.layer.0.attention.self.key.bias': (333056, 128, (128,)),
                   'bert.encoder.layer.0.attention.self.value.bias': (333184, 128, (128,)),
                   'bert.encoder.layer.0.attention.output.dense.bias': (333312, 128, (128,)),
                   'bert.encoder.layer.0.attention.output.LayerNorm.weight': (333440, 128, (128,)),
                   'bert.encoder.layer.0.attention.output.LayerNorm.bias': (333568, 128, (128,)),
                   'bert.encoder.layer.0.intermediate.dense.bias': (333696, 256, (256,)),
                   'bert.encoder.layer.0.output.dense.bias': (333952, 128, (128,)),
                   'bert.encoder.layer.0.output.LayerNorm.weight': (334080, 128, (128,)),
                   'bert.encoder.layer.0.output.LayerNorm.bias': (334208, 128, (128,)),
                   'bert.encoder.layer.1.attention.self.query.bias': (334336, 128, (128,)),
                   'bert.encoder.layer.1.attention.self.key.bias': (334464, 128, (128,)),
                   'bert.encoder.layer.1.attention.self.value.bias': (334592, 128, (128,)),
                   'bert.encoder.layer.1.attention.output.dense.bias': (334720, 128, (128,)),
                   'bert.encoder.layer.1.attention.output.LayerNorm.weight': (334848, 128, (128,)),
                   'bert.encoder.layer.1.attention.output.LayerNorm.bias': (334976, 128, (128,)),
                   'bert.encoder.layer.1.intermediate.dense.bias': (335104, 256, (256,)),
                   'bert.encoder.layer.1.output.dense.bias': (335360, 128, (128,)),
                   'bert.encoder.layer.1.output.LayerNorm.weight': (335488, 128, (128,)),
                   'bert.encoder.layer.1.output.LayerNorm.bias': (335616, 128, (128,)),
                   'bert.pooler.dense.bias': (335744, 128, (128,)),
                   'bert.img_embedding.bias': (335872, 128, (128,)),
                   'bert.location_embeds.bias': (336000, 128, (128,)),
                   'next_action.linear.bias': (336128, 5, (5,)),
                   'mlmhead.predictions.bias': (336192, 97, (97,)),
                   'mlmhead.predictions.transform.dense.bias': (336320, 128, (128,)),
                   'mlmhead.predictions.transform.LayerNorm.weight': (336448, 128, (128,)),
                   'mlmhead.predictions.transform.LayerNorm.bias': (336576, 128, (128,)),
                   'token_head.0.bias': (336704, 11, (11,))},
           'layer_ranges': [[(16768, 147840), (332928, 334336)], [(147840, 278912), (334336, 335744)]],
           'head_ranges': [(278912, 295296), (314240, 332672), (335744, 335872), (336128, 336768)],
           'shard_atoms': [(0, 16768), (16768, 147840), (147840, 278912), (278912, 295296), (295296, 314240), (314240, 332672),
                           (332672, 332928), (332928, 334336), (334336, 335744), (335744, 335872), (335872, 336128),
                           (336128, 336768)],
           'shard_launch_ranges': [[(278912, 295296), (314240, 332672), (335744, 335872), (336128, 336768)],
                                   [(147840, 278912), (334336, 335744)], [(16768, 147840), (332928, 334336)],
                                   [(0, 16768), (295296, 314240), (332672, 332928), (335872, 336128)]],
           'fp32_spans': [(0, 16768), (332672, 336768)],
           'mirror_only': ['bert.encoder.layer.0.attention.output.dense.weight',
                           'bert.encoder.layer.0.attention.self.key.weight', 'bert.encoder.layer.0.attention.self.query.weight',
                           'bert.encoder.layer.0.attention.self.value.weight', 'bert.encoder.layer.0.intermediate.dense.weight',
                           'bert.encoder.layer.0.output.dense.weight', 'bert.encoder.layer.1.attention.output.dense.weight',
                           'bert.encoder.layer.1.attention.self.key.weight', 'bert.encoder.layer.1.attention.self.query.weight',
                           'bert.encoder.layer.1.attention.self.value.weight', 'bert.encoder.layer.1.intermediate.dense.weight',
                           'bert.encoder.layer.1.output.dense.weight', 'bert.img_embedding.weight',
                           'bert.location_embeds.weight', 'bert.pooler.dense.weight',
                           'mlmhead.predictions.transform.dense.weight', 'next_action.linear.weight', 'token_head.0.weight'],
           'transposes': [('bert.encoder.layer.0.attention.self.query.weight', (384, 128), (128, 384)),
                          ('bert.encoder.layer.0.attention.output.dense.weight', (128, 128), (128, 128)),
                          ('bert.encoder.layer.0.intermediate.dense.weight', (256, 128), (128, 256)),
                          ('bert.encoder.layer.0.output.dense.weight', (128, 256), (256, 128)),
                          ('bert.encoder.layer.1.attention.self.query.weight', (384, 128), (128, 384)),
                          ('bert.encoder.layer.1.attention.output.dense.weight', (128, 128), (128, 128)),
                          ('bert.encoder.layer.1.intermediate.dense.weight', (256, 128), (128, 256)),
                          ('bert.encoder.layer.1.output.dense.weight', (128, 256), (256, 128)),
                          ('bert.pooler.dense.weight', (128, 128), (128, 128)),
                          ('mlmhead.predictions.transform.dense.weight', (128, 128), (128, 128)),
                          ('bert.embeddings.word_embeddings.weight', (97, 128), (128, 128)),
                          ('token_head.0.weight', (11, 128), (128, 64)), ('next_action.linear.weight', (5, 128), (128, 64))]},
 'img_layernorm': {'total': 337024,
                   'n_decay': 332672,
                   'off': {'bert.embeddings.word_embeddings.weight': (0, 12416, (97, 128)),
                           'bert.embeddings.position_embeddings.weight': (12416, 4096, (32, 128)),
                           'bert.embeddings.token_type_embeddings.weight': (16512, 256, (2, 128)),
                           'bert.encoder.layer.0.attention.self.query.weight': (16768, 16384, (128, 128)),
                           'bert.encoder.layer.0.attention.self.key.weight': (33152, 16384, (128, 128)),
                           'bert.encoder.layer.0.attention.self.value.weight': (49536, 16384, (128, 128)),
                           'bert.encoder.layer.0.attention.output.dense.weight': (65920, 16384, (128, 128)),
                           'bert.encoder.layer.0.intermediate.dense.weight': (82304, 32768, (256, 128)),
                           'bert.encoder.layer.0.output.dense.weight': (115072, 32768, (128, 256)),
                           'bert.encoder.layer.1.attention.self.query.weight': (147840, 16384, (128, 128)),
                           'bert.encoder.layer.1.attention.self.key.weight': (164224, 16384, (128, 128)),
                           'bert.encoder.layer.1.attention.self.value.weight': (180608, 16384, (128, 128)),
                           'bert.encoder.layer.1.attention.output.dense.weight': (196992, 16384, (128, 128)),
                           'bert.encoder.layer.1.intermediate.dense.weight': (213376, 32768, (256, 128)),
                           'bert.encoder.layer.1.output.dense.weight': (246144, 32768, (128, 256)),
                           'bert.pooler.dense.weight': (278912, 16384, (128, 128)),
                           'bert.img_embedding.weight': (295296, 2560, (128, 20)),
                           'bert.location_embeds.weight': (297856, 16384, (128, 128)),
                           'next_action.linear.weight': (314240, 640, (5, 128)),
                           'mlmhead.predictions.transform.dense.weight': (314880, 16384, (128, 128)),
                           'token_head.0.weight': (331264, 1408, (11, 128)),
                           'bert.embeddings.LayerNorm.weight': (332672, 128, (128,)),
                           'bert.embeddings.LayerNorm.bias': (332800, 128, (128,)),
                           'bert.encoder.layer.0.attention.self.query.bias': (332928, 128, (128,)),
                           'bert.encoder.layer.0.attention.self.key.bias': (333056, 128, (128,)),
                           'bert.encoder.layer.0.attention.self.value.bias': (333184, 128, (128,)),
                           'bert.encoder.layer.0.attention.output.dense.bias': (333312, 128, (128,)),
                           'bert.encoder.layer.0.attention.output.LayerNorm.weight': (333440, 128, (128,)),
                           'bert.encoder.layer.0.attention.output.LayerNorm.bias': (333568, 128, (128,)),
                           'bert.encoder.layer.0.intermediate.dense.bias': (333696, 256, (256,)),
                           'bert.encoder.layer.0.output.dense.bias': (333952, 128, (128,)),
                           'bert.encoder.layer.0.output.LayerNorm.weight': (334080, 128, (128,)),
                           'bert.encoder.layer.0.output.LayerNorm.bias': (334208, 128, (128,)),
                           'bert.encoder.layer.1.attention.self.query.bias': (334336, 128, (128,)),
                           'bert.encoder.layer.1.attention.self.key.bias': (334464, 128, (128,)),
                           'bert.encoder.layer.1.attention.self.value.bias': (334592, 128, (128,)),
                           'bert.encoder.layer.1.attention.output.dense.bias': (334720, 128, (128,)),
                           'bert.encoder.layer.1.attention.output.LayerNorm.weight': (334848, 128, (128,)),
                           'bert.encoder.layer.1.attention.output.LayerNorm.bias': (334976, 128, (128,)),
                           'bert.encoder.layer.1.intermediate.dense.bias': (335104, 256, (256,)),
                           'bert.encoder.layer.1.output.dense.bias': (335360, 128, (128,)),
                           'bert.encoder.layer.1.output.LayerNorm.weight': (335488, 128, (128,)),
                           'bert.encoder.layer.1.output.LayerNorm.bias': (335616, 128, (128,)),
                           'bert.pooler.dense.bias': (335744, 128, (128,)),
                           'bert.img_embedding.bias': (335872, 128, (128,)),
                           'bert.location_embeds.bias': (336000, 128, (128,)),
                           'bert.LayerNorm.weight': (336128, 128, (128,)),
                           'bert.LayerNorm.bias': (336256, 128, (128,)),
                           'next_action.linear.bias': (336384, 5, (5,)),
                           'mlmhead.predictions.bias': (336448, 97, (97,)),
                           'mlmhead.predictions.transform.dense.bias': (336576, 128, (128,)),
                           'mlmhead.predictions.transform.LayerNorm.weight': (336704, 128, (128,)),
                           'mlmhead.predictions.transform.LayerNorm.bias': (336832, 128, (128,)),
                           'token_head.0.bias': (336960, 11, (11,))},
                   'layer_ranges': [[(16768, 147840), (332928, 334336)], [(147840, 278912), (334336, 335744)]],
                   'head_ranges': [(278912, 295296), (314240, 332672), (335744, 335872), (336384, 337024)],
                   'shard_atoms': [(0, 16768), (16768, 147840), (147840, 278912), (278912, 295296), (295296, 314240),
                                   (314240, 332672), (332672, 332928), (332928, 334336), (334336, 335744), (335744, 335872),
                                   (335872, 336384), (336384, 337024)],
                   'shard_launch_ranges': [[(278912, 295296), (314240, 332672), (335744, 335872), (336384, 337024)],
                                           [(147840, 278912), (334336, 335744)], [(16768, 147840), (332928, 334336)],
                                           [(0, 16768), (295296, 314240), (332672, 332928), (335872, 336384)]],
                   'fp32_spans': [(0, 16768), (332672, 337024)],
                   'mirror_only': ['bert.encoder.layer.0.attention.output.dense.weight',
                                   'bert.encoder.layer.0.attention.self.key.weight',
                                   'bert.encoder.layer.0.attention.self.query.weight',
                                   'bert.encoder.layer.0.attention.self.value.weight',
                                   'bert.encoder.layer.0.intermediate.dense.weight', 'bert.encoder.layer.0.output.dense.weight',
                                   'bert.encoder.layer.1.attention.output.dense.weight',
                                   'bert.encoder.layer.1.attention.self.key.weight',
                                   'bert.encoder.layer.1.attention.self.query.weight',
                                   'bert.encoder.layer.1.attention.self.value.weight',
                                   'bert.encoder.layer.1.intermediate.dense.weight', 'bert.encoder.layer.1.output.dense.weight',
                                   'bert.img_embedding.weight', 'bert.location_embeds.weight', 'bert.pooler.dense.weight',
                                   'mlmhead.predictions.transform.dense.weight', 'next_action.linear.weight',
                                   'token_head.0.weight'],
                   'transposes': [('bert.encoder.layer.0.attention.self.query.weight', (384, 128), (128, 384)),
                                  ('bert.encoder.layer.0.attention.output.dense.weight', (128, 128), (128, 128)),
                                  ('bert.encoder.layer.0.intermediate.dense.weight', (256, 128), (128, 256)),
                                  ('bert.encoder.layer.0.output.dense.weight', (128, 256), (256, 128)),
                                  ('bert.encoder.layer.1.attention.self.query.weight', (384, 128), (128, 384)),
                                  ('bert.encoder.layer.1.attention.output.dense.weight', (128, 128), (128, 128)),
                                  ('bert.encoder.layer.1.intermediate.dense.weight', (256, 128), (128, 256)),
                                  ('bert.encoder.layer.1.output.dense.weight', (128, 256), (256, 128)),
                                  ('bert.pooler.dense.weight', (128, 128), (128, 128)),
                                  ('mlmhead.predictions.transform.dense.weight', (128, 128), (128, 128)),
                                  ('bert.embeddings.word_embeddings.weight', (97, 128), (128, 128)),
                                  ('token_head.0.weight', (11, 128), (128, 64)),
                                  ('next_action.linear.weight', (5, 128), (128, 64))]},
 'untied': {'total': 349568,
            'n_decay': 345472,
            'off': {'bert.embeddings.word_embeddings.weight': (0, 12800, (100, 128)),
                    'bert.embeddings.position_embeddings.weight': (12800, 4096, (32, 128)),
                    'bert.embeddings.token_type_embeddings.weight': (16896, 256, (2, 128)),
                    'bert.encoder.layer.0.attention.self.query.weight': (17152, 16384, (128, 128)),
                    'bert.encoder.layer.0.attention.self.key.weight': (33536, 16384, (128, 128)),
                    'bert.encoder.layer.0.attention.self.value.weight': (49920, 16384, (128, 128)),
                    'bert.encoder.layer.0.attention.output.dense.weight': (66304, 16384, (128, 128)),
                    'bert.encoder.layer.0.intermediate.dense.weight': (82688, 32768, (256, 128)),
                    'bert.encoder.layer.0.output.dense.weight': (115456, 32768, (128, 256)),
                    'bert.encoder.layer.1.attention.self.query.weight': (148224, 16384, (128, 128)),
                    'bert.encoder.layer.1.attention.self.key.weight': (164608, 16384, (128, 128)),
                    'bert.encoder.layer.1.attention.self.value.weight': (180992, 16384, (128, 128)),
                    'bert.encoder.layer.1.attention.output.dense.weight': (197376, 16384, (128, 128)),
                    'bert.encoder.layer.1.intermediate.dense.weight': (213760, 32768, (256, 128)),
                    'bert.encoder.layer.1.output.dense.weight': (246528, 32768, (128, 256)),
                    'bert.pooler.dense.weight': (279296, 16384, (128, 128)),
                    'bert.img_embedding.weight': (295680, 2560, (128, 20)),
                    'bert.location_embeds.weight': (298240, 16384, (128, 128)),
                    'next_action.linear.weight': (314624, 640, (5, 128)),
                    'mlmhead.predictions.transform.dense.weight': (315264, 16384, (128, 128)),
                    'mlmhead.predictions.decoder.weight': (331648, 12416, (97, 128)),
                    'token_head.0.weight': (344064, 1408, (11, 128)),
                    'bert.embeddings.LayerNorm.weight': (345472, 128, (128,)),
                    'bert.embeddings.LayerNorm.bias': (345600, 128, (128,)),
                    'bert.encoder.layer.0.attention.self.query.bias': (345728, 128, (128,)),
                    'bert.encoder.layer.0.attention.self.key.bias': (345856, 128, (128,)),
                    'bert.encoder.layer.0.attention.self.value.bias': (345984, 128, (128,)),
                    'bert.encoder.layer.0.attention.output.dense.bias': (346112, 128, (128,)),
                    'bert.encoder.layer.0.attention.output.LayerNorm.weight': (346240, 128, (128,)),
                    'bert.encoder.layer.0.attention.output.LayerNorm.bias': (346368, 128, (128,)),
                    'bert.encoder.layer.0.intermediate.dense.bias': (346496, 256, (256,)),
                    'bert.encoder.layer.0.output.dense.bias': (346752, 128, (128,)),
                    'bert.encoder.layer.0.output.LayerNorm.weight': (346880, 128, (128,)),
                    'bert.encoder.layer.0.output.LayerNorm.bias': (347008, 128, (128,)),
                    'bert.encoder.layer.1.attention.self.query.bias': (347136, 128, (128,)),
                    'bert.encoder.layer.1.attention.self.key.bias': (347264, 128, (128,)),
                    'bert.encoder.layer.1.attention.self.value.bias': (347392, 128, (128,)),
                    'bert.encoder.layer.1.attention.output.dense.bias': (347520, 128, (128,)),
                    'bert.encoder.layer.1.attention.output.LayerNorm.weight': (347648, 128, (128,)),
                    'bert.encoder.layer.1.attention.output.LayerNorm.bias': (347776, 128, (128,)),
                    'bert.encoder.layer.1.intermediate.dense.bias': (347904, 256, (256,)),
                    'bert.encoder.layer.1.output.dense.bias': (348160, 128, (128,)),
                    'bert.encoder.layer.1.output.LayerNorm.weight': (348288, 128, (128,)),
                    'bert.encoder.layer.1.output.LayerNorm.bias': (348416, 128, (128,)),
                    'bert.pooler.dense.bias': (348544, 128, (128,)),
                    'bert.img_embedding.bias': (348672, 128, (128,)),
                    'bert.location_embeds.bias': (348800, 128, (128,)),
                    'next_action.linear.bias': (348928, 5, (5,)),
                    'mlmhead.predictions.bias': (348992, 97, (97,)),
                    'mlmhead.predictions.transform.dense.bias': (349120, 128, (128,)),
                    'mlmhead.predictions.transform.LayerNorm.weight': (349248, 128, (128,)),
                    'mlmhead.predictions.transform.LayerNorm.bias': (349376, 128, (128,)),
                    'token_head.0.bias': (349504, 11, (11,))},
            'layer_ranges': [[(17152, 148224), (345728, 347136)], [(148224, 279296), (347136, 348544)]],
            'head_ranges': [(279296, 295680), (314624, 345472), (348544, 348672), (348928, 349568)],
            'shard_atoms': [(0, 17152), (17152, 148224), (148224, 279296), (279296, 295680), (295680, 314624), (314624, 345472),
                            (345472, 345728), (345728, 347136), (347136, 348544), (348544, 348672), (348672, 348928),
                            (348928, 349568)],
            'shard_launch_ranges': [[(279296, 295680), (314624, 345472), (348544, 348672), (348928, 349568)],
                                    [(148224, 279296), (347136, 348544)], [(17152, 148224), (345728, 347136)],
                                    [(0, 17152), (295680, 314624), (345472, 345728), (348672, 348928)]],
            'fp32_spans': [(0, 17152), (345472, 349568)],
            'mirror_only': ['bert.encoder.layer.0.attention.output.dense.weight',
                            'bert.encoder.layer.0.attention.self.key.weight',
                            'bert.encoder.layer.0.attention.self.query.weight',
                            'bert.encoder.layer.0.attention.self.value.weight',
                            'bert.encoder.layer.0.intermediate.dense.weight', 'bert.encoder.layer.0.output.dense.weight',
                            'bert.encoder.layer.1.attention.output.dense.weight',
                            'bert.encoder.layer.1.attention.self.key.weight',
                            'bert.encoder.layer.1.attention.self.query.weight',
                            'bert.encoder.layer.1.attention.self.value.weight',
                            'bert.encoder.layer.1.intermediate.dense.weight', 'bert.encoder.layer.1.output.dense.weight',
                            'bert.img_embedding.weight', 'bert.location_embeds.weight', 'bert.pooler.dense.weight',
                            'mlmhead.predictions.decoder.weight', 'mlmhead.predictions.transform.dense.weight',
                            'next_action.linear.weight', 'token_head.0.weight'],
            'transposes': [('bert.encoder.layer.0.attention.self.query.weight', (384, 128), (128, 384)),
                           ('bert.encoder.layer.0.attention.output.dense.weight', (128, 128), (128, 128)),
                           ('bert.encoder.layer.0.intermediate.dense.weight', (256, 128), (128, 256)),
                           ('bert.encoder.layer.0.output.dense.weight', (128, 256), (256, 128)),
                           ('bert.encoder.layer.1.attention.self.query.weight', (384, 128), (128, 384)),
                           ('bert.encoder.layer.1.attention.output.dense.weight', (128, 128), (128, 128)),
                           ('bert.encoder.layer.1.intermediate.dense.weight', (256, 128), (128, 256)),
                           ('bert.encoder.layer.1.output.dense.weight', (128, 256), (256, 128)),
                           ('bert.pooler.dense.weight', (128, 128), (128, 128)),
                           ('mlmhead.predictions.transform.dense.weight', (128, 128), (128, 128)),
                           ('mlmhead.predictions.decoder.weight', (97, 128), (128, 128)),
                           ('token_head.0.weight', (11, 128), (128, 64)), ('next_action.linear.weight', (5, 128), (128, 64))]},
 'trunk': {'total': 317696,
           'n_decay': 314240,
           'off': {'bert.embeddings.word_embeddings.weight': (0, 12416, (97, 128)),
                   'bert.embeddings.position_embeddings.weight': (12416, 4096, (32, 128)),
                   'bert.embeddings.token_type_embeddings.weight': (16512, 256, (2, 128)),
                   'bert.encoder.layer.0.attention.self.query.weight': (16768, 16384, (128, 128)),
                   'bert.encoder.layer.0.attention.self.key.weight': (33152, 16384, (128, 128)),
                   'bert.encoder.layer.0.attention.self.value.weight': (49536, 16384, (128, 128)),
                   'bert.encoder.layer.0.attention.output.dense.weight': (65920, 16384, (128, 128)),
                   'bert.encoder.layer.0.intermediate.dense.weight': (82304, 32768, (256, 128)),
                   'bert.encoder.layer.0.output.dense.weight': (115072, 32768, (128, 256)),
                   'bert.encoder.layer.1.attention.self.query.weight': (147840, 16384, (128, 128)),
                   'bert.encoder.layer.1.attention.self.key.weight': (164224, 16384, (128, 128)),
                   'bert.encoder.layer.1.attention.self.value.weight': (180608, 16384, (128, 128)),
                   'bert.encoder.layer.1.attention.output.dense.weight': (196992, 16384, (128, 128)),
                   'bert.encoder.layer.1.intermediate.dense.weight': (213376, 32768, (256, 128)),
                   'bert.encoder.layer.1.output.dense.weight': (246144, 32768, (128, 256)),
                   'bert.pooler.dense.weight': (278912, 16384, (128, 128)),
                   'bert.img_embedding.weight': (295296, 2560, (128, 20)),
                   'bert.location_embeds.weight': (297856, 16384, (128, 128)),
                   'bert.embeddings.LayerNorm.weight': (314240, 128, (128,)),
                   'bert.embeddings.LayerNorm.bias': (314368, 128, (128,)),
                   'bert.encoder.layer.0.attention.self.query.bias': (314496, 128, (128,)),
                   'bert.encoder.layer.0.attention.self.key.bias': (314624, 128, (128,)),
                   'bert.encoder.layer.0.attention.self.value.bias': (314752, 128, (128,)),
                   'bert.encoder.layer.0.attention.output.dense.bias': (314880, 128, (128,)),
                   'bert.encoder.layer.0.attention.output.LayerNorm.weight': (315008, 128, (128,)),
                   'bert.encoder.layer.0.attention.output.LayerNorm.bias': (315136, 128, (128,)),
                   'bert.encoder.layer.0.intermediate.dense.bias': (315264, 256, (256,)),
                   'bert.encoder.layer.0.output.dense.bias': (315520, 128, (128,)),
                   'bert.encoder.layer.0.output.LayerNorm.weight': (315648, 128, (128,)),
                   'bert.encoder.layer.0.output.LayerNorm.bias': (315776, 128, (128,)),
                   'bert.encoder.layer.1.attention.self.query.bias': (315904, 128, (128,)),
                   'bert.encoder.layer.1.attention.self.key.bias': (316032, 128, (128,)),
                   'bert.encoder.layer.1.attention.self.value.bias': (316160, 128, (128,)),
                   'bert.encoder.layer.1.attention.output.dense.bias': (316288, 128, (128,)),
                   'bert.encoder.layer.1.attention.output.LayerNorm.weight': (316416, 128, (128,)),
                   'bert.encoder.layer.1.attention.output.LayerNorm.bias': (316544, 128, (128,)),
                   'bert.encoder.layer.1.intermediate.dense.bias': (316672, 256, (256,)),
                   'bert.encoder.layer.1.output.dense.bias': (316928, 128, (128,)),
                   'bert.encoder.layer.1.output.LayerNorm.weight': (317056, 128, (128,)),
                   'bert.encoder.layer.1.output.LayerNorm.bias': (317184, 128, (128,)),
                   'bert.pooler.dense.bias': (317312, 128, (128,)),
                   'bert.img_embedding.bias': (317440, 128, (128,)),
                   'bert.location_embeds.bias': (317568, 128, (128,))},
           'layer_ranges': [[(16768, 147840), (314496, 315904)], [(147840, 278912), (315904, 317312)]],
           'head_ranges': None,
           'shard_atoms': [(0, 16768), (16768, 147840), (147840, 278912), (278912, 314496), (314496, 315904), (315904, 317312),
                           (317312, 317696)],
           'shard_launch_ranges': [[(147840, 278912), (315904, 317312)], [(16768, 147840), (314496, 315904)],
                                   [(0, 16768), (278912, 314496), (317312, 317696)]],
           'fp32_spans': [(0, 16768), (314240, 317696)],
           'mirror_only': ['bert.encoder.layer.0.attention.output.dense.weight',
                           'bert.encoder.layer.0.attention.self.key.weight', 'bert.encoder.layer.0.attention.self.query.weight',
                           'bert.encoder.layer.0.attention.self.value.weight', 'bert.encoder.layer.0.intermediate.dense.weight',
                           'bert.encoder.layer.0.output.dense.weight', 'bert.encoder.layer.1.attention.output.dense.weight',
                           'bert.encoder.layer.1.attention.self.key.weight', 'bert.encoder.layer.1.attention.self.query.weight',
                           'bert.encoder.layer.1.attention.self.value.weight', 'bert.encoder.layer.1.intermediate.dense.weight',
                           'bert.encoder.layer.1.output.dense.weight', 'bert.img_embedding.weight',
                           'bert.location_embeds.weight', 'bert.pooler.dense.weight'],
           'transposes': [('bert.encoder.layer.0.attention.self.query.weight', (384, 128), (128, 384)),
                          ('bert.encoder.layer.0.attention.output.dense.weight', (128, 128), (128, 128)),
                          ('bert.encoder.layer.0.intermediate.dense.weight', (256, 128), (128, 256)),
                          ('bert.encoder.layer.0.output.dense.weight', (128, 256), (256, 128)),
                          ('bert.encoder.layer.1.attention.self.query.weight', (384, 128), (128, 384)),
                          ('bert.encoder.layer.1.attention.output.dense.weight', (128, 128), (128, 128)),
                          ('bert.encoder.layer.1.intermediate.dense.weight', (256, 128), (128, 256)),
                          ('bert.encoder.layer.1.output.dense.weight', (128, 256), (256, 128)),
                          ('bert.pooler.dense.weight', (128, 128), (128, 128))]}}


# (recorded the same way) the transposed head copy each pair of the transpose batch writes, None for a layer's own four
_LAYER_DST = [None] * 8
HEAD_DST = {"plain": _LAYER_DST + ["pool", "tr", "dec", "tok", "act"], "img_layernorm": _LAYER_DST + ["pool", "tr", "dec", "tok", "act"],
            "untied": _LAYER_DST + ["pool", "tr", "dec", "tok", "act"], "trunk": _LAYER_DST + ["pool"]}


@pytest.mark.parametrize("variant", VARIANTS)
def test_engine_tables_match_the_recorded_literals(variant, monkeypatch):
    got, want = _describe(_engine(variant), monkeypatch), dict(EXPECTED[variant], head_dst=HEAD_DST[variant])
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


def test_the_plain_configuration_has_the_recorded_sizes(monkeypatch):
    got = _describe(_engine("plain"), monkeypatch)
    assert (got["total"], got["n_decay"]) == (336768, 332672)
    counts = [len(got[k]) for k in ("shard_atoms", "shard_launch_ranges", "fp32_spans", "mirror_only")]
    assert counts == [12, 4, 2, 18]


def test_trunk_state_is_one_declared_class():
    st = training.TrunkState()
    assert all(getattr(st, name) is None for name in training.TrunkState.__slots__)
    with pytest.raises(AttributeError):
        st.not_a_declared_field = 1
    assert not hasattr(st, "__dict__")
    for name in ("mask", "mode", "e", "x0", "layers", "d_history"):
        assert name in training.TrunkState.__slots__
    # the fp32 step fills the same class: it defines none of its own and builds its state through the training module
    assert training_f32.training is training
    with open(os.path.splitext(training_f32.__file__)[0] + ".py") as fh:
        src = fh.read()
    assert not any(isinstance(n, ast.ClassDef) for n in ast.walk(ast.parse(src)))
    assert "return training.TrunkState(" in src and "__dict__" not in src


@pytest.mark.parametrize("module", [training, training_f32])
def test_no_locals_and_no_method_bolted_on_after_a_class_body(module):
    with open(os.path.splitext(module.__file__)[0] + ".py") as fh:
        src = fh.read()
    assert "locals()" not in src
    tree = ast.parse(src)
    classes = {n.name for n in tree.body if isinstance(n, ast.ClassDef)}
    functions = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    for node in tree.body:
        if isinstance(node, ast.Assign):
            for tgt in node.targets:
                bolted = (isinstance(tgt, ast.Attribute) and isinstance(tgt.value, ast.Name) and tgt.value.id in classes
                          and isinstance(node.value, (ast.Name, ast.Lambda))
                          and (isinstance(node.value, ast.Lambda) or node.value.id in functions))
                assert not bolted, "line %d assigns a function to %s.%s" % (node.lineno, tgt.value.id, tgt.attr)
