"""The one table behind ImageCaptioning.pack, TrainEngine.bind_inference and TrainEngine._matrices (vitcap_amd.weights.weights_table)
against the three things it has to agree with: the C struct, the checkpoint layout, and the operand list the training engine kept
before the table existed (tests/golden/train_matrices.json, recorded from TrainEngine._matrices() of the commit before it)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from vitcap_amd import weights as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _leaves(struct, at=()):
    """Paths of every pointer leaf of a ctypes structure, arrays and nested structures walked."""
    out = []
    for name, typ in struct._fields_:
        if issubclass(typ, C.Array):
            for i in range(typ._length_):
                out += _leaves(typ._type_, at + (name, i))
        elif issubclass(typ, C.Structure):
            out += _leaves(typ, at + (name,))
        else:
            assert typ is C.c_void_p, (at, name, typ)
            out.append(at + (name,))
    return out


def test_table_names_every_leaf_of_the_weights_struct_once():
    from vitcap_amd import _lib as L
    want = _leaves(L.Weights)
    got = [f.path for f in W.weights_table()]
    assert len(want) == C.sizeof(L.Weights) // C.sizeof(C.c_void_p)
    assert len(got) == len(set(got)), 'a field is listed twice'
    assert sorted(got, key=repr) == sorted(want, key=repr)
    assert W.VOCAB_PAD == L.VOCAB_PAD and W.VOCAB == L.VOCAB
    # a tied field points at a field listed before it, of the same kind and padding
    by_path = {f.path: (i, f) for i, f in enumerate(W.weights_table())}
    for i, f in enumerate(W.weights_table()):
        if f.tied_to:
            j, src = by_path[f.tied_to]
            assert j < i and (src.kind, src.pad) == (f.kind, f.pad)
            assert (f.keys, src.keys) == ((W.TIED_DST,), (W.TIED_SRC,))


def test_table_keys_exist_with_shapes_of_the_declared_kind():
    spec = W.state_dict_spec()
    seen = []
    for f in W.weights_table():
        assert f.kind in ('mat', 'vec') and len(f.keys) in (1, 3), f.path
        for k in f.keys:
            assert k in spec, (f.path, k)
        seen += f.keys
        shapes = [spec[k][0] for k in f.keys]
        assert all(s[1:] == shapes[0][1:] for s in shapes), f.path          # concatenated along dim 0
        n = sum(int(np.prod(s)) for s in shapes)
        if f.kind == 'mat':
            N, K = f.rows_cols(spec)
            assert len(shapes[0]) >= 2 and N * K == n and K % 64 == 0, f.path       # rows of bf16, whole 64-element k-steps
            assert (f.name is None) == f.optional, f.path                   # the training engine keeps a pair of every matrix it binds
            if f.shape is not None:
                assert tuple(f.shape) == (N, K), f.path
        else:
            squeezed = [d for d in shapes[0] if d != 1]
            assert f.name is None and (len(squeezed) == 1 or f.shape is not None), f.path
            if f.shape is not None:
                assert int(np.prod(f.shape)) == n, f.path
        if f.pad is not None:
            assert f.pad == W.VOCAB_PAD and shapes[0][0] == W.VOCAB, f.path
        assert f.optional == f.keys[0].startswith('module.bert.extra_embeddings.'), f.path
    assert len(seen) == len(set(seen)), 'a checkpoint tensor feeds two fields'


@pytest.mark.parametrize('tied', [True, False])
def test_training_matrices_are_those_of_the_parent(tied):
    from vitcap_amd.train import TrainEngine

    class _Model(object):
        tie_weights = tied
    eng = TrainEngine.__new__(TrainEngine)          # _matrices() reads nothing but model.tie_weights
    eng.model = _Model()
    got = [tuple(m) for m in eng._matrices()]
    with open(os.path.join(GOLD, 'train_matrices.json')) as f:
        want = [tuple(m) for m in json.load(f)['tied' if tied else 'untied']]
    assert len(got) == len(set(got))
    assert set(want) <= set(got), sorted(set(want) - set(got))
    assert got == want          # and nothing else, in the cast table's order
