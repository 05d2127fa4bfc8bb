"""Which generate() options every analysis call refuses BY NAME before it touches a device: the whole matrix, cell by cell.

A cell (call, override) is "refused" iff the call raises NotImplementedError whose text holds the option's name; anything else --
another exception, or reaching pack() -- is "not refused".  The expected matrix is a literal, recorded from the tree before the
refusals were folded into one table (vitcap_amd/model.py _REFUSED); its inconsistencies (caption_with_maps lets tag_visible through to
its greedy pass, the stepwise calls never look at do_sample, ...) are pinned as they are."""
import pytest
import torch

from vitcap_amd.model import ImageCaptioning
from vitcap_amd.regions import grid_regions

OVERRIDES = {'': {}, 'B': dict(num_beams=3), 'C': dict(use_cbs=True), 'T': dict(tag_visible=2), 'S': dict(do_sample=True),
             'G': dict(use_graph=True), 'R': dict(repetition_penalty=1.2)}
NAMES = {'B': 'num_beams', 'C': 'use_cbs', 'T': 'tag_visible', 'S': 'do_sample', 'G': 'use_graph', 'R': 'repetition_penalty'}

IMG = torch.zeros(2, 1)
CAP = torch.tensor([[101, 5, 102] + [0] * 17] * 2)
VIS = torch.ones(2, 578, dtype=torch.bool)
VIS4 = torch.ones(4, 578, dtype=torch.bool)
PRESENT = torch.ones(2, 24, 24, dtype=torch.bool)
BOXES = grid_regions(2)

# call -> (the options it refuses by name, the call)
CALLS = {
    'generate(visible=)': ('BCT', lambda m, **kw: m.generate(IMG, visible=VIS, **kw)),
    'generate_multi(2, visible=)': ('BCT', lambda m, **kw: m.generate_multi(IMG, 2, visible=VIS4, **kw)),
    'score_masked(one_pass=False)': ('BCT', lambda m, **kw: m.score_masked(IMG, CAP, VIS, one_pass=False, **kw)),
    'generate_beam(3, visible=)': ('CTSG', lambda m, **kw: m.generate_beam(IMG, 3, visible=VIS, **kw)),
    'caption_regions_beam(.., 3)': ('CTSG', lambda m, **kw: m.caption_regions_beam(IMG, BOXES, 3, **kw)),
    'caption_with_regions_beam(.., 3)': ('CTSG', lambda m, **kw: m.caption_with_regions_beam(IMG, BOXES, 3, **kw)),
    'score(one_pass=True)': ('BCTSR', lambda m, **kw: m.score(IMG, CAP, one_pass=True, **kw)),
    'score_masked': ('BCTSR', lambda m, **kw: m.score_masked(IMG, CAP, VIS, **kw)),
    'attention_maps': ('BCTSR', lambda m, **kw: m.attention_maps(IMG, CAP, **kw)),
    'alternatives': ('BCTSR', lambda m, **kw: m.alternatives(IMG, CAP, **kw)),
    'occlusion_maps': ('BCTSR', lambda m, **kw: m.occlusion_maps(IMG, CAP, **kw)),
    'visual_gain': ('BCTSR', lambda m, **kw: m.visual_gain(IMG, CAP, **kw)),
    'caption_with_maps': ('BCS', lambda m, **kw: m.caption_with_maps(IMG, **kw)),
    'caption_with_alternatives': ('BCS', lambda m, **kw: m.caption_with_alternatives(IMG, **kw)),
    'caption_with_occlusion': ('BCS', lambda m, **kw: m.caption_with_occlusion(IMG, **kw)),
    'caption_regions': ('BCTS', lambda m, **kw: m.caption_regions(IMG, BOXES, **kw)),
    'caption_with_regions': ('BCTS', lambda m, **kw: m.caption_with_regions(IMG, BOXES, **kw)),
    'tag_patches': ('BCTSG', lambda m, **kw: m.tag_patches(IMG, PRESENT, **kw)),
    'caption_patches': ('BCTSG', lambda m, **kw: m.caption_patches(IMG, PRESENT, **kw)),
    'caption_crops': ('BCTSG', lambda m, **kw: m.caption_crops(IMG, BOXES, **kw)),
    'caption_with_crops': ('BCTSG', lambda m, **kw: m.caption_with_crops(IMG, BOXES, **kw)),
    'encoder_attention': ('BCTSG', lambda m, **kw: m.encoder_attention(IMG, **kw)),
    'tag_rollout': ('BCTSG', lambda m, **kw: m.tag_rollout(IMG, **kw)),
    'caption_with_rollout': ('BCTSG', lambda m, **kw: m.caption_with_rollout(IMG, **kw)),
    'score_patches': ('BCTSGR', lambda m, **kw: m.score_patches(IMG, CAP, PRESENT, **kw)),
    'rollout_maps': ('BCTSGR', lambda m, **kw: m.rollout_maps(IMG, CAP, **kw)),
    # nothing is on the slot: the RuntimeError that says so comes before every refusal
    'score_encoded': ('', lambda m, **kw: m.score_encoded(CAP, **kw)),
}


class ReachedPack(Exception):
    """The call got past its host-side refusals."""


@pytest.fixture(scope='module')
def model():
    m = ImageCaptioning(tie_weights=True).eval()

    def pack(*a, **kw):
        raise ReachedPack()
    m.pack = pack                      # a model without a device: nothing is ever packed
    return m


def test_the_table_has_the_27_calls():
    assert len(CALLS) == 27 and len(OVERRIDES) == 7
    assert all(set(letters) <= set(NAMES) for letters, _ in CALLS.values())


@pytest.mark.parametrize('opt', list(OVERRIDES))
@pytest.mark.parametrize('name', list(CALLS))
def test_cell(model, name, opt):
    letters, call = CALLS[name]
    refused = False
    try:
        call(model, **OVERRIDES[opt])
    except NotImplementedError as e:
        refused = bool(opt) and NAMES[opt] in str(e)
    except Exception:
        pass
    assert refused == (opt in letters if opt else False), (name, OVERRIDES[opt])
    assert model._packed is None and model._engine is None


@pytest.mark.parametrize('opt', list(OVERRIDES))
def test_score_encoded_reports_the_empty_slot_first(model, opt):
    with pytest.raises(RuntimeError, match='no encoded images on slot'):
        model.score_encoded(CAP, **OVERRIDES[opt])
