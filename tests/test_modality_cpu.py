"""One modality alone, host side: the CPU composition (tests/modality_ref.py) against the imported reference's fixtures
(tests/golden/modality_*.npz, make_golden_modality.py) and against the joint oracle, and the argument rules of
``model.normalize_modality``.  No GPU."""
import numpy as np
import pytest
import torch

import modality_ref as M
from diffsheg_amd.config import get_config
from diffsheg_amd.model import MODALITIES, normalize_modality
from diffsheg_amd.synthetic import make_inputs
from oracle import denoiser_ref
from util import synthetic_sd

ORACLE_GATE = 2e-6            # of the output range: tests/test_oracle_golden.py's gate


@pytest.mark.parametrize("ds", ["show", "beat"])
def test_composition_evaluations_match_reference(ds):
    c = M.fixture_case(ds)
    cfg, f, inp, B = c["cfg"], c["f"], c["inp"], c["B"]
    for tag in ("k0", "k14"):
        with torch.no_grad():
            eps = M.gesture_eps(c["sd"], cfg, inp["x_T"], torch.full((B,), int(f[f"{tag}_t"]), dtype=torch.long), inp["audio_emb"],
                                inp["person_id"], inp["pretrain_aud_feat"], c["track"])
        ref = torch.from_numpy(f[f"{tag}_eps_ges"])
        e = float((eps[..., :cfg.split_pos] - ref).abs().max())
        print(f"[modality cpu {ds} {tag}] max|eps_ges - ref| = {e:.3e} (range {float(ref.abs().max()):.3g})")
        assert e <= ORACLE_GATE * max(float(ref.abs().max()), 1.0), (tag, e)
        assert not eps[..., cfg.split_pos:].any()


@pytest.mark.parametrize("ds", ["show", "beat"])
def test_composition_loops_match_reference(ds):
    c = M.fixture_case(ds)
    cfg, f, G = c["cfg"], c["f"], c["cfg"].split_pos
    assert c["draws"] == int(f["ddim_draws"]) == 26
    assert c["masked_draws"] == int(f["masked_draws"])
    for name, x in (("ddim", c["comp_ddim"]), ("masked", c["comp_masked"])):
        ref = torch.from_numpy(f[f"{name}_final_ges"])
        e, scale = float((x[..., :G] - ref).abs().max()), float(ref.abs().max())
        print(f"[modality cpu {ds} {name}] max|x_ges - ref| = {e:.3e} (range {scale:.3g})")
        assert e <= ORACLE_GATE * scale, (name, e, scale)
        assert torch.equal(x[..., G:], c["track"])            # the expression columns of the result are the given track


@pytest.mark.parametrize("ds", ["show", "beat"])
def test_given_the_joint_estimate_the_composition_is_the_joint_oracle(ds):
    cfg, sd = get_config(ds), synthetic_sd(ds)
    B, G = 2, cfg.split_pos
    inp = make_inputs(cfg, B, seed=9)
    t = torch.full((B,), 560, dtype=torch.long)
    c1, c2 = torch.tensor(4.9), torch.tensor(4.8)
    with torch.no_grad():
        joint, parts = denoiser_ref.unidiffuser(sd, cfg, inp["x_T"], t, c1, c2, inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"],
                                                return_parts=True)
        ges = M.gesture_eps(sd, cfg, inp["x_T"], t, inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"], parts["expr_x0"])
        exp = M.expression_eps(sd, cfg, inp["x_T"], t, inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"])
    assert torch.equal(ges[..., :G], joint[..., :G])
    assert torch.equal(exp[..., G:], joint[..., G:])
    assert not ges[..., G:].any() and not exp[..., :G].any()


def test_normalize_modality_accepts():
    tr = torch.zeros(2, 5, 7)
    assert MODALITIES == {"both": 0, "expression": 1, "gesture": 2}
    assert normalize_modality() == 0 and normalize_modality(None) == 0 and normalize_modality("both") == 0 and normalize_modality(0) == 0
    assert normalize_modality("expression") == 1 and normalize_modality(1) == 1 and normalize_modality(np.int64(1)) == 1
    assert normalize_modality("gesture", tr) == 2 and normalize_modality(2, tr, 2, 5, 7) == 2
    assert normalize_modality("gesture", tr.double(), batch=2, frames=5, expression_dim=7) == 2
    assert normalize_modality("both", None, unidiffuser=False, same_overlap_noisy=True) == 0


@pytest.mark.parametrize("kw", [
    dict(modality="face"), dict(modality=3), dict(modality=-1), dict(modality=1.0), dict(modality=True),
    dict(modality="gesture"),                                                        # no track
    dict(modality="gesture", expression=torch.zeros(2, 5, 6), expression_dim=7),     # wrong width
    dict(modality="gesture", expression=torch.zeros(2, 4, 7), frames=5),             # wrong frame count
    dict(modality="gesture", expression=torch.zeros(3, 5, 7), batch=2),              # wrong batch
    dict(modality="gesture", expression=torch.zeros(5, 7)),                          # not [B, T, E]
    dict(modality="gesture", expression=torch.zeros(2, 5, 7, dtype=torch.long)),     # not floating point
    dict(modality="gesture", expression=[[0.0]]),                                    # not a tensor
    dict(modality="expression", expression=torch.zeros(2, 5, 7)),                    # a track without the gesture modality
    dict(modality="both", expression=torch.zeros(2, 5, 7)),
    dict(modality="expression", unidiffuser=False),                                  # single MotionTransformer
    dict(modality="gesture", expression=torch.zeros(2, 5, 7), unidiffuser=False),
    dict(modality="expression", same_overlap_noisy=True),                            # the saved tails describe all channels
    dict(modality="gesture", expression=torch.zeros(2, 5, 7), same_overlap_noisy=True),
])
def test_normalize_modality_refuses(kw):
    with pytest.raises(ValueError):
        normalize_modality(**kw)
