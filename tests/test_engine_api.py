"""The Python view of include/vame.h is single-sourced: the ABI constants live
in vame._lib and every module re-exports those objects, and each predictor
(`_p`) method of Engine is its plain counterpart's signature plus one
predictor parameter.  Imports only: no engine, no device work."""
import inspect

import pytest

from vame import _lib, bipred, engine, mvp, partition, shard


def test_abi_constants_have_one_home():
    for mod in (engine, partition, bipred, shard):
        assert mod.MODES is _lib.MODES, mod.__name__
    assert _lib.MODES == ("FULL_2CP", "FULL_3CP", "HALF_2CP", "HALF_3CP")
    for mod in (partition, bipred):
        assert mod.MAX_PENALTY is _lib.MAX_PENALTY, mod.__name__
    assert _lib.MAX_PENALTY == 1 << 40
    assert mvp.PER is _lib.CUS_PER_CTU
    assert _lib.CUS_PER_CTU == (201, 284)
    bits = (engine.MODE_2CP, engine.MODE_3CP, engine.MODE_FULL, engine.MODE_HALF)
    assert bits == (_lib.MODE_2CP, _lib.MODE_3CP, _lib.MODE_FULL, _lib.MODE_HALF) == (1, 2, 4, 8)


PAIRS = (("affine_search", "affine_search_p", "preds", 2), ("bipred_refine", "bipred_refine_p", "preds", 2),
         ("affine_mc_bi", "affine_mc_p", "preds", 2), ("affine_me_seeded", "affine_me_seeded_p", "mvp", 6),
         ("bipred", "bipred_p", "mvp", 5))


@pytest.mark.parametrize("plain,pred,name,at", PAIRS, ids=[p[1] for p in PAIRS])
def test_predictor_method_is_its_counterpart_plus_one_parameter(plain, pred, name, at):
    """`at`: the predictor's position among the parameters (self = 0)."""
    want = inspect.signature(getattr(engine.Engine, plain))
    got = inspect.signature(getattr(engine.Engine, pred))
    params = list(got.parameters.values())
    assert params[at].name == name
    assert params[at].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    del params[at]
    assert got.replace(parameters=params) == want
