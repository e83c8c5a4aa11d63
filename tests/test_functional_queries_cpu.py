"""How src/ops/functional.py asks the library shape questions and builds its descriptors, on CPU tensors against a recording stand-in
for the library (tests/_functional_replay.py): no GPU, no built library.

One cache (_QUERY_CACHE) behind every question, one clear; a launch wrapper is never answered from it; a cached question refuses tensors;
and every descriptor, plain argument and answer equals what tests/golden/functional_descs.json holds -- recorded by
tools/gen_golden_functional.py from the same call lists before the questions were moved onto one mechanism and the descriptors onto
one builder each."""
import gc
import json
import os
import sys
import weakref

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _functional_replay as R      # noqa: E402
from src.ops import functional as K      # noqa: E402

QUESTIONS = list(R.QUESTIONS)
FFI_QUESTIONS = [q for q in QUESTIONS if q not in R.NO_FFI]
S2_DOWN = dict(k=3, Ci=64, Cj=64, gather_i=True, grid_g=(16, 16), grid_d=(8, 8))


def test_the_question_list_is_the_sixteen():
    assert len(QUESTIONS) == 16 and all(callable(getattr(K, q)) for q in QUESTIONS)


def test_no_memoised_launch():
    """conv_s2_wgrad_f32 twice on the same three tensors: two launches (dW += twice), and the operands are not kept alive"""
    with R.stubbed(K, {"*": 1, "mi_conv_s2_wgrad_f32_workspace": 64}) as stub:
        P, Q, dW = R.act(2, 16, 16, 64), R.act(2, 8, 8, 64), torch.zeros(9 * 64 * 64)
        assert K.conv_s2_wgrad_f32(P, Q, dW, **S2_DOWN) is True
        assert K.conv_s2_wgrad_f32(P, Q, dW, **S2_DOWN) is True
        assert stub.names().count("mi_conv_s2_wgrad_f32") == 2, stub.names()
        assert stub.names().count("mi_conv_s2_wgrad_f32_supported") == 1          # the question behind it is asked once
        ref = weakref.ref(P)
        del P
        gc.collect()
        assert ref() is None
    for attr in ("cache_clear", "cache_info", "__wrapped__"):
        assert not hasattr(K.conv_s2_wgrad_f32, attr), attr


def test_s2_wgrad_supported_is_cached():
    args = (16, 3, 128, 128, False, (32, 32), (16, 16), 1)
    with R.stubbed(K) as stub:
        assert K.s2_wgrad_supported(*args) is True and K.s2_wgrad_supported(*args) is True
        assert stub.names() == ["mi_conv_s2_wgrad_tr_supported"]


@pytest.mark.parametrize("name", QUESTIONS)
def test_one_cache_one_clear(name):
    """two identical calls cost the FFI calls of one; after _QUERY_CACHE.clear() and flipped answers the next call gives the new answer"""
    settings, shapes = R.QUESTIONS[name]
    args, kw = shapes[0]
    fn = getattr(K, name)
    lo, hi = settings[0], settings[-1]
    with R.stubbed(K, hi) as stub:
        first = fn(*args, **kw)
        once = len(stub.calls)
        assert fn(*args, **kw) == first and len(stub.calls) == once
        assert (once == 0) == (name in R.NO_FFI)
        stub.answers = dict(lo)
        assert fn(*args, **kw) == first and len(stub.calls) == once               # still the cached answer
        K._QUERY_CACHE.clear()
        flipped = fn(*args, **kw)
        if name in R.NO_FFI:
            assert flipped == first and not stub.calls
        else:
            assert flipped != first and len(stub.calls) > once, (first, flipped)
            assert type(flipped) is type(first)


def test_positional_and_keyword_forms_agree():
    with R.stubbed(K):
        for ks, ci, co in ((3, 3, 128), (3, 3, 96), (1, 4, 64), (5, 3, 64)):
            assert K.small_cin_supported(ks, ci, co, wgrad=True) == K.small_cin_supported(ks, ci, co, True)
            assert K.small_cin_supported(ks, ci, co, wgrad=False) == K.small_cin_supported(ks, ci, co)
        assert K.small_cin_supported(3, 3, 128, wgrad=True) is True and K.small_cin_supported(3, 3, 96, wgrad=True) is False
        assert K.fast3x3_supported(16, 16, 16, 512, 256, K1=256) == K.fast3x3_supported(16, 16, 16, 512, 256, 256)


@pytest.mark.parametrize("name", QUESTIONS)
def test_tensors_are_refused(name):
    """a cached question handed a tensor -- bare, inside a tuple, by keyword -- raises and names itself: a launch wrapper decorated by
    accident fails on its first call instead of skipping launches"""
    args, kw = R.QUESTIONS[name][1][0]
    fn = getattr(K, name)
    t = torch.zeros(2, 2)
    with R.stubbed(K) as stub:
        for bad_args, bad_kw in (((t,) + args[1:], kw), (((t, 1),) + args[1:], kw), (args, dict(kw, extra=t))):
            with pytest.raises(TypeError, match=name):
                fn(*bad_args, **bad_kw)
        assert not stub.calls and not K._QUERY_CACHE


def test_missing_is_not_none():
    """an answer of None is an answer: asked once"""
    with R.stubbed(K, {"*": None}) as stub:
        d = K._conv_desc(2, 8, 8, 128, 128, 3)
        assert K._query("mi_conv3x3_pw_tile", d) is None and K._query("mi_conv3x3_pw_tile", d) is None
        assert len(stub.calls) == 1


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "functional_descs.json")) as f:
        return json.load(f)


def _same(got, want):
    got = json.loads(json.dumps(got))                      # tuples -> lists, as the file holds them
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, f"{g[0]}:\n got  {g[1:]}\n want {w[1:]}"


def test_answers_and_question_descriptors_unchanged(golden):
    """every question over the cfg-2 (B = 16), MNIST, two-source and refused shapes, under every answer setting (0 / 1, 0 / a size, the four
    conv x wgrad combinations, the tiles): the FFI calls with their descriptor fields, and the returned value with its type"""
    _same(R.replay_questions(K), golden["questions"])


def test_wrapper_descriptors_unchanged(golden):
    """every launch wrapper that builds a descriptor, arm by arm: entry points, descriptor fields and plain arguments, in order"""
    _same(R.replay_wrappers(K), golden["wrappers"])
