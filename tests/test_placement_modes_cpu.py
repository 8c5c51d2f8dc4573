"""CPU: the four object-placement modes of the engine (``placement``, ``variant_placements``, ``transform``, ``variant_transforms``;
DESIGN.md 6k, 6l, 6n, 6o) are mutually exclusive and resolved when a site asks -- which message a mix of them
raises, that every mode is refused under a frame shard by name, and the order of the checks.  No kernel is launched."""
import itertools
import types

import pytest

PL = (((1, 0),), ((0, 1),))  # two objects, one frame
TR = ((2, 1, 2, 1, False, False, 8, 8, ((0, 0),)),) * 2
# highest precedence first: a mix raises the message of its first member
VALUES = (("variant_transforms", (TR, TR)), ("transform", TR), ("variant_placements", (PL, PL)), ("placement", PL))
MIX = {"variant_transforms": "variant_transforms is set together with placement / variant_placements / transform",
       "transform": "transform is set together with placement / variant_placements",
       "variant_placements": "variant_placements and placement are both set"}
SHARD = {attr: subject + " not combine with the frame shard" for attr, subject in (
    ("variant_transforms", "variant_transforms do"), ("transform", "a transform does"),
    ("variant_placements", "variant_placements do"), ("placement", "a placement does"))}
MASKS = [None, None]  # the refusals come before anything reads a mask
SUBSETS = [c for n in (2, 3, 4) for c in itertools.combinations(VALUES, n)]


def _engine(variants=2):
    from mvoc_amd.unet import I2VGenXLUNet
    eng = I2VGenXLUNet(device="cpu")
    eng.variants = variants
    return eng


def test_every_mix_raises_the_message_of_its_highest_precedence_member():
    assert len(SUBSETS) == 11
    eng = _engine()
    for subset in SUBSETS:
        for attr, value in subset:
            setattr(eng, attr, value)  # (plain attributes: nothing is refused at assignment)
        with pytest.raises(RuntimeError) as e:
            eng.place_kw(MASKS, 8, 8)
        assert str(e.value).startswith(MIX[subset[0][0]]), (subset, str(e.value))
        for attr, _ in subset:
            setattr(eng, attr, None)
    assert eng.place_kw(MASKS, 8, 8) == {}


@pytest.mark.parametrize("attr,value", VALUES)
def test_every_mode_is_refused_under_a_frame_shard_by_name(attr, value):
    eng = _engine()
    setattr(eng, attr, value)
    eng.shard = types.SimpleNamespace(rank=0, world=1)
    for call in (lambda: eng.place_kw(MASKS, 8, 8), lambda: eng.pnp_batch(3 + 2 * eng.variants, MASKS)):
        with pytest.raises(RuntimeError, match="frame shard") as e:
            call()
        assert str(e.value).startswith(SHARD[attr]), str(e.value)


@pytest.mark.parametrize("attr,value", VALUES)
def test_the_shard_is_checked_before_the_object_count(attr, value):
    eng = _engine()
    setattr(eng, attr, value)
    with pytest.raises(RuntimeError, match="the hooks carry 3 masks"):  # two objects in the value, three masks
        eng.place_kw([None] * 3, 8, 8)
    eng.shard = types.SimpleNamespace(rank=0, world=1)
    with pytest.raises(RuntimeError) as e:
        eng.place_kw([None] * 3, 8, 8)
    assert str(e.value).startswith(SHARD[attr]), str(e.value)


@pytest.mark.parametrize("attr,value", [v for v in VALUES if v[0].startswith("variant_")])
def test_the_variant_count_is_checked_before_the_object_count(attr, value):
    eng = _engine(variants=3)
    setattr(eng, attr, value)
    with pytest.raises(RuntimeError, match=f"{attr} holds 2 .*, the call 3 variants"):
        eng.place_kw([None] * 3, 8, 8)
