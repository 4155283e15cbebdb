"""CPU: Segment Anything's wiring.  The float64 restatement (tests/sam_restatement.py) is pinned against transformers' SamModel and against
the recorded fixture; the checkpoint importer and the host surface of detector='sam' are checked without a GPU."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sam_cases as C  # noqa: E402
import sam_restatement as R  # noqa: E402
from cartoonsegmentation_amd.nets import sam as S  # noqa: E402
from cartoonsegmentation_amd.weights import StateDictWeights, SynthWeights  # noqa: E402


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("kw,boxes,seed", [(C.CFG_A, C.BOXES_A, C.SEED_A), (C.CFG_B, C.BOXES_B, C.SEED_B)], ids=['A', 'B'])
def test_restatement_matches_transformers_sam_model(kw, boxes, seed):
    """float64 against float64 on the same graph: only the summation order differs -> 1e-9 relative in max-norm"""
    pytest.importorskip("transformers")
    cfg = S.SamConfig(**kw)
    sd = R.random_state_dict(S.sam_param_shapes(cfg), seed)
    x = torch.as_tensor(np.random.default_rng(seed + 10).standard_normal((1, 3, cfg.image, cfg.image)))
    low, iou = R.Model(sd, cfg).forward(x, boxes)
    hl, hi = R.hf_forward(R.hf_model(cfg, sd), x, boxes)
    assert low.shape == (len(boxes), 4 * cfg.grid, 4 * cfg.grid) and float(hl.abs().max()) > 0.05      # unit-scale logits, not 5e-5
    print('logits', _rel(low, hl), 'iou', _rel(iou, hi))
    assert _rel(low, hl) < 1e-9 and _rel(iou, hi) < 1e-9


def test_restatement_matches_the_recorded_sam_model_outputs():
    """the same pin without transformers: tests/golden/sam_tiny.npz holds SamModel's float64 outputs for config A"""
    z = np.load(C.GOLDEN)
    cfg = S.SamConfig(**C.CFG_A)
    sd = R.random_state_dict(S.sam_param_shapes(cfg), int(z['seed']))
    low, iou = R.Model(sd, cfg).forward(torch.as_tensor(C.prepared(z['image_u8'])), z['boxes'])
    assert _rel(low, torch.as_tensor(z['low_res_logits'])) < 1e-9 and _rel(iou, torch.as_tensor(z['iou'])) < 1e-9


def test_key_map_covers_transformers_parameters():
    pytest.importorskip("transformers")
    cfg = S.SamConfig(**C.CFG_A)
    sd = R.random_state_dict(S.sam_param_shapes(cfg), 3)
    m = R.hf_model(cfg, sd)                                             # (asserts: nothing unexpected, nothing missing)
    assert set(R.to_hf_state_dict(sd)) == set(m.state_dict())


class _Tracking(StateDictWeights):
    def __init__(self, sd):
        super().__init__(sd)
        self.seen = set()

    def get(self, name, shape, kind):
        self.seen.add(name)
        return super().get(name, shape, kind)


def test_checkpoint_importer_round_trips_every_key():
    cfg = S.SamConfig(**C.CFG_A)
    sd = S.synth_state_dict(SynthWeights('sam.'), cfg)
    assert set(sd) == set(S.sam_param_shapes(cfg)) and all(tuple(sd[k].shape) == tuple(v) for k, v in S.sam_param_shapes(cfg).items())
    ws = _Tracking({k: torch.from_numpy(v) for k, v in sd.items()})     # as torch.load hands them over
    enc, dec = S.build_sam_encoder(ws, cfg, 1), S.build_sam_decoder(ws, cfg, 2)
    S.prompt_constants(ws, cfg)
    unread = {k for k in sd if k not in ws.seen}
    multimask = {k for k in unread if k.startswith(tuple('mask_decoder.output_hypernetworks_mlps.%d.' % i for i in (1, 2, 3)))}
    assert unread - multimask == {k for k in sd if k.startswith(S.UNUSED_KEYS)}, sorted(unread)
    # the same programs from the synthetic source directly: every value arrived unchanged
    enc2, dec2 = S.build_sam_encoder(SynthWeights('sam.'), cfg, 1), S.build_sam_decoder(SynthWeights('sam.'), cfg, 2)
    for a, b in ((enc, enc2), (dec, dec2)):
        assert np.array_equal(a.serialise()[2], b.serialise()[2]) and [o['kind'] for o in a.ops] == [o['kind'] for o in b.ops]
    got = S.infer_config(ws.sd)
    assert {k: getattr(got, k) for k in C.CFG_A} == C.CFG_A


@pytest.mark.parametrize("preset", ['vit_b', 'vit_l', 'vit_h'])
def test_presets_are_inferred_from_shapes(preset):
    class Shape:
        def __init__(self, shape):
            self.shape = shape
    cfg = S.SamConfig(preset)
    assert (cfg.window, cfg.patch, cfg.image, cfg.out_chans, cfg.grid) == (14, 16, 1024, 256, 64)
    got = S.infer_config({k: Shape(v) for k, v in S.sam_param_shapes(cfg).items()})
    assert S.preset_of(got) == preset and (got.window, got.image, got.mlp_dim, got.head_dim) == (14, 1024, 4 * cfg.embed, cfg.head_dim)


def test_relative_position_table_of_the_wrong_length_is_refused():
    cfg = S.SamConfig(**C.CFG_A)
    sd = S.synth_state_dict(SynthWeights('sam.'), cfg)
    sd['image_encoder.blocks.0.attn.rel_pos_w'] = np.zeros((2 * 7 - 1, cfg.head_dim), np.float32)    # the global length in a window block
    with pytest.raises(ValueError, match='relative position table'):
        S.build_sam_encoder(StateDictWeights(sd), cfg, 1)


def test_dense_positional_encoding_matches_the_restatement():
    cfg = S.SamConfig(**C.CFG_A)
    sd = R.random_state_dict(S.sam_param_shapes(cfg), 4)
    pe = S.dense_pe(sd['prompt_encoder.pe_layer.positional_encoding_gaussian_matrix'], cfg.grid)
    ref = R.Model(sd, cfg).dense_pe()[0].permute(1, 2, 0).numpy()
    assert np.abs(pe - ref).max() < 1e-6


# ---- host surface ------------------------------------------------------------------------------------------------------------------------------
def test_reference_import_of_apply_sam_resolves():
    from sam import apply_sam
    from cartoonsegmentation_amd.sam import apply_sam as ours
    assert apply_sam is ours


def test_sam_yaml_keys_load_and_other_detectors_still_raise(monkeypatch):
    from cartoonsegmentation_amd import kenburns as K
    yaml_like = {'inpaint_type': 'ldm', 'detector': 'sam', 'num_frame': 75, 'playback': True, 'dof_speed': 50, 'depth_field': False, 'max_size': 1024,
                 'ldm_inpaint_size': 1024, 'ldm_inpaint_options': {'steps': 32}, 'sd_img2img_url': 'http://127.0.0.1:7860/sdapi/v1/img2img',
                 'mask_refine_kwargs': {'refine_method': 'refinenet_isnet', 'refine_size': 720}, 'depth_est': 'leres', 'depth_est_size': 640,
                 'det_ckpt': 'models/AnimeInstanceSegmentation/rtmdetl_e60.ckpt', 'det_size': 640, 'pred_score_thr': 0.3, 'refine_crf': False,
                 'depth_factor': 1}
    cfg = K.build_kenburns_cfg(yaml_like)
    assert cfg.detector == 'sam' and cfg.sam_ckpt == 'models/sam/sam_vit_h_4b8939.pth' and cfg.max_size == 1024
    assert K.build_kenburns_cfg(dict(yaml_like, sam_ckpt='x.pth')).sam_ckpt == 'x.pth'
    # set_detector without a device: the selection logic on a bare object
    pipe = object.__new__(K.KenBurnsPipeline)
    pipe.cfg, pipe.device, pipe.animeinsseg, pipe.sam = cfg, 'cuda:0', object(), None
    for other in ('maskrcnn', 'yolo'):
        with pytest.raises(NotImplementedError):
            pipe.set_detector(other)
    made = []
    monkeypatch.setattr(K, 'Sam', lambda path, device=None: made.append((path, device)) or 'the predictor')
    pipe.set_detector('sam')
    assert pipe.sam == 'the predictor' and made == [('models/sam/sam_vit_h_4b8939.pth', 'cuda:0')] and pipe.detector == 'sam'
    pipe.set_detector('animeinsseg')
    assert pipe.detector == 'animeinsseg'


def test_checkpoint_path_resolution(monkeypatch):
    from cartoonsegmentation_amd import sam as M
    monkeypatch.delenv('CSM_SAM_CKPT', raising=False)
    assert M.resolve_ckpt() == 'models/sam/sam_vit_h_4b8939.pth' and M.resolve_ckpt('a.pth') == 'a.pth'
    monkeypatch.setenv('CSM_SAM_CKPT', '/w/sam_vit_b.pth')
    assert M.resolve_ckpt('a.pth') == '/w/sam_vit_b.pth'
    monkeypatch.setenv('CSM_SYNTHETIC_WEIGHTS', '0')
    with pytest.raises(FileNotFoundError):
        M.load_sam_weights('/nonexistent/sam.pth')
    monkeypatch.delenv('CSM_SAM_CKPT')
    monkeypatch.setenv('CSM_SYNTHETIC_WEIGHTS', '1')
    monkeypatch.setenv('CSM_SAM_PRESET', 'vit_b')
    ws, cfg = M.load_sam_weights('/nonexistent/sam.pth')
    assert isinstance(ws, SynthWeights) and ws.prefix == 'sam.' and S.preset_of(cfg) == 'vit_b'


def test_masks_near_zero_are_rare_for_the_end_to_end_cases():
    """the premise of tests/test_gpu_sam.py's mask comparison, on the restatement alone: at most 0.5 % of a mask's pixels have a float64
    logit within 1e-4 max|logit| of zero"""
    import sam_e2e_cases as E
    for case in E.CASES:
        logits, _ = E.reference(case)
        for k in range(logits.shape[0]):
            band = 1e-4 * float(logits[k].abs().max())
            assert float((logits[k].abs() <= band).double().mean()) <= 0.005, (case['name'], k)
