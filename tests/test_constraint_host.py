"""Constrained decoding without a GPU (include/flm_gpu.h: flm_dfa, flm_dfa_validate; host/sampler.cpp constrain_logits / dfa_next through lib/libflm_host.so; capi.Dfa):
the validator's rules one by one, step 0's host restatement against an independent NumPy mask on the bit patterns, delta against a dict, Dfa.from_choices' paths, and the
text format's round trip."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import capi, synth
from constraint_util import SIZES, Dfa, cycle3, delta, edge_lists, ends, np_mask, pairs, table, wide
from shape_util import bits

V = 288


def test_the_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(graft.ROOT, "include", "flm_gpu.h")).read()
    lib = capi.lib()
    for sym in ("flm_dfa_validate", "flm_constraint_set", "flm_constraint_arm", "flm_op_constrain_rows"):
        assert sym + "(" in hdr and sym in capi.SYMBOLS and hasattr(lib, sym)
    assert capi.DFA_STATES_MAX == int(re.search(r"#define FLM_DFA_STATES_MAX\s+(\d+)", hdr).group(1))
    assert "#define FLM_DFA_EDGES_MAX  (1 << 24)" in hdr and capi.DFA_EDGES_MAX == 1 << 24


def test_validate_accepts_the_test_automata():
    for d in (cycle3(V), pairs(V), ends(V, 2), wide(V)):
        capi.dfa_validate(d, V)
    assert cycle3(V).n_states == 3 and cycle3(V).n_edges == V and pairs(V).n_edges == 16 and wide(V).n_edges == V


def _bad(dfa, message, vocab=V):
    with pytest.raises(capi.FlmError, match="flm error -1") as e:
        capi.dfa_validate(dfa, vocab)
    assert message in str(e.value), (message, str(e.value))


def test_validate_rejects_each_rule_with_its_own_message():
    _bad(Dfa([0, 2, 2, 3], [1, 5, 7], [0, 1, 2]), "a state has no edge")
    _bad(Dfa([0, 3], [1, 5, 5], [0, 0, 0]), "listed twice")
    _bad(Dfa([0, 3], [1, 9, 5], [0, 0, 0]), "strictly ascending")
    _bad(Dfa([0, 2], [1, V], [0, 0]), "edge token outside [0, vocab)")
    _bad(Dfa([0, 2], [-1, 4], [0, 0]), "edge token outside [0, vocab)")
    _bad(Dfa([0, 1, 2], [1, 4], [0, 2]), "edge_next outside [0, n_states)")
    _bad(Dfa([0, 1, 2], [1, 4], [-1, 0]), "edge_next outside [0, n_states)")
    _bad(Dfa([1, 2], [1, 4], [0, 0]), "row_ptr must start at 0 and end at n_edges")
    _bad(Dfa([0, 1], [1, 4], [0, 0]), "row_ptr must start at 0 and end at n_edges")
    _bad(Dfa([0, 2, 1, 3], [1, 4, 6], [0, 0, 0]), "non-decreasing")
    _bad(Dfa([0], [], []), "n_states outside")
    _bad(Dfa(np.arange(capi.DFA_STATES_MAX + 2), np.zeros(capi.DFA_STATES_MAX + 1), np.zeros(capi.DFA_STATES_MAX + 1)), "n_states outside")
    _bad(Dfa([0, 0], [], []), "n_edges outside")
    assert capi.lib().flm_dfa_validate(None, V) == -1


@pytest.mark.parametrize("n", SIZES)
def test_fh_constrain_equals_the_numpy_mask(n):
    L = (np.random.default_rng(n).standard_normal(n) * 4).astype(np.float32)
    L[::7] = np.float32(-0.0); L[3 % n] = -np.inf
    for name, toks in edge_lists(n).items():
        got, want = capi.constrain_host(L, toks), np_mask(L, toks)
        assert np.array_equal(bits(got), bits(want)), (n, name)
    assert np.array_equal(bits(capi.constrain_host(L, edge_lists(n)["all"])), bits(L))


def test_fh_dfa_next_equals_the_dict():
    for d in (cycle3(V), pairs(V), ends(V, 2), wide(V)):
        tab = table(d)
        rng = np.random.default_rng(1)
        for q in range(d.n_states):
            toks = list(d.edges(q)[0][:4]) + [int(x) for x in rng.integers(0, V, 24)]
            for t in toks:
                assert capi.dfa_next_host(d, q, t) == delta(tab, q, t), (q, t)
    p = pairs(V)
    free = next(t for t in range(V) if (0, t) not in table(p))
    assert capi.dfa_next_host(p, 0, free) == 0                     # no edge: the state stays


def _spellings(d, pieces, end_id):
    """every string a path from state 0 to the final state spells (the automaton of from_choices is acyclic up to the final loop)"""
    final, out = d.n_states - 1, set()

    def walk(q, text):
        for t, nx in zip(*d.edges(q)):
            if int(t) == end_id:
                assert int(nx) == final
                out.add(text)
            else:
                assert int(nx) != final
                walk(int(nx), text + pieces[int(t)])
    walk(0, "")
    return out


def test_from_choices_spells_exactly_the_choices():
    tk = synth.make_tokenizer(320)
    pieces = list(tk.texts)
    choices = ["yes", "no", "not", "maybe", "may"]
    d = Dfa.from_choices(pieces, choices, end_id=2)
    capi.dfa_validate(d, 320)
    assert _spellings(d, pieces, 2) == set(choices)
    final = d.n_states - 1
    assert list(d.edges(final)[0]) == [2] and list(d.edges(final)[1]) == [final]
    # pieces of several characters: every segmentation of a choice is a path, nothing else is
    pieces2 = ["", "", "<end>", "y", "e", "s", "ye", "es", "yes", "n", "o", "no", "x", "yesx"]
    d2 = Dfa.from_choices(pieces2, ["yes", "no"], end_id=2)
    capi.dfa_validate(d2, len(pieces2))
    assert _spellings(d2, pieces2, 2) == {"yes", "no"}
    assert sorted(int(t) for t in d2.edges(0)[0]) == [3, 6, 8, 9, 11]          # y, ye, yes, n, no


def test_save_load_round_trips(tmp_path):
    for i, d in enumerate((cycle3(V), pairs(V), ends(V, 2), Dfa.from_choices(list(synth.make_tokenizer(320).texts), ["to", "tea"], 2))):
        path = str(tmp_path / f"a{i}.dfa")
        d.save(path)
        assert open(path).readline().split() == ["flm-dfa", "1", str(d.n_states)]
        e = Dfa.load(path)
        assert np.array_equal(e.row_ptr, d.row_ptr) and np.array_equal(e.edge_token, d.edge_token) and np.array_equal(e.edge_next, d.edge_next)
    # the loader sorts: the same edges in reverse order
    path = str(tmp_path / "rev.dfa")
    lines = open(str(tmp_path / "a1.dfa")).read().splitlines()
    open(path, "w").write("\n".join([lines[0]] + lines[:0:-1]) + "\n")
    e = Dfa.load(path)
    assert np.array_equal(e.edge_token, pairs(V).edge_token) and np.array_equal(e.edge_next, pairs(V).edge_next)
    open(path, "w").write("not-a-dfa 1 3\n")
    with pytest.raises(ValueError):
        Dfa.load(path)
