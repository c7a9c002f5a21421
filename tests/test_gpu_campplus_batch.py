"""`CAMPPlus.forward_ragged` on the GPU: all clips of tests/golden/campplus.npz (outputs of the REFERENCE's own CAMPPlus class on the oracle's
seeded weights, tools/make_golden_campplus.py) in ONE ragged call, every row held to the bar tests/test_gpu_campplus.py holds the per-clip path
to (5e-4 absolute, against the reference class -- not against the code under test): in golden order, reversed, and with a column budget that
splits the FCM head into three groups.  The largest difference between a batched row and the per-clip row is printed (DESIGN.md section 19 keeps
the figure; nothing gates on it: a GEMM's path depends on its row count).  `forward` itself is unchanged: a (2, T, 80) input is bitwise the
concatenation of two single calls."""
import os

import numpy as np
import pytest
import torch

from oracle import campplus_oracle as CO
from tools.make_golden_campplus import LENGTHS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-4


@pytest.fixture(scope="module")
def model():
    from indextts_amd.campplus import CAMPPlus
    m = CAMPPlus(feat_dim=80, embedding_size=192, device=DEV)
    m.load_state_dict(CO.synth_weights())
    return m.eval()


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "campplus.npz"))
    return [torch.from_numpy(z[f"feats{i}"]) for i in range(len(LENGTHS))], [torch.from_numpy(z[f"style{i}"]) for i in range(len(LENGTHS))]


def _held(y, styles, order, what):
    assert y.shape == (len(order), 192)
    for row, i in enumerate(order):
        err = float((y[row].cpu() - styles[i]).abs().max())
        print(f"CAMPPlus.forward_ragged ({what}) T={LENGTHS[i]}: max|d| vs the reference class {err:.2e}")
        assert err <= TOL, f"{what}: clip {i} (T = {LENGTHS[i]}) is {err:.2e} from the reference class"


def test_one_ragged_call_vs_reference_class(model, golden):
    feats, styles = golden
    order = list(range(len(LENGTHS)))
    y = model.forward_ragged(feats)
    assert model.last_head_groups == [order]                            # the default budget: one head group
    _held(y, styles, order, "golden order")
    rev = order[::-1]
    y_rev = model.forward_ragged([feats[i] for i in rev])
    _held(y_rev, styles, rev, "reversed")
    per_clip = torch.cat([model(f.unsqueeze(0)) for f in feats], 0)
    d = max(float((y - per_clip).abs().max()), float((y_rev.flip(0) - per_clip).abs().max()))
    print(f"CAMPPlus.forward_ragged vs forward per clip: largest |batched - per-clip| {d:.2e} (style rms {float(per_clip.pow(2).mean().sqrt()):.2f})")


def test_head_split_into_three_groups_by_the_column_budget(model, golden):
    from indextts_amd.campplus import head_col_bytes
    feats, styles = golden
    budget = head_col_bytes(LENGTHS[1])          # 57 fits, 57 + 130 does not, 263 alone is over the budget: a group of its own
    y = model.forward_ragged(feats, col_budget_bytes=budget)
    assert len(model.last_head_groups) >= 3 and model.last_head_groups == [[0], [1], [2]]
    _held(y, styles, list(range(len(LENGTHS))), "three head groups")


def test_one_prompt_empty_list_and_refusals(model, golden):
    feats, styles = golden
    _held(model.forward_ragged(feats[:1]), styles, [0], "one prompt")
    assert model.forward_ragged([]).shape == (0, 192)
    with pytest.raises(ValueError):
        model.forward_ragged([feats[0], torch.zeros(3, 80)])            # T >= 4, as forward requires
    with pytest.raises(ValueError):
        model.forward_ragged([torch.zeros(50, 64)])


def test_forward_is_still_the_per_clip_loop(model, golden):
    feats, _ = golden
    T = LENGTHS[0]
    x = torch.stack([feats[0], feats[1][:T]], 0)
    both = model(x)
    assert both.shape == (2, 192)
    assert torch.equal(both, torch.cat([model(x[:1]), model(x[1:])], 0))
