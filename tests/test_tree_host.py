"""Tree draft-and-verify without a GPU (include/flm_gpu.h): flm_tree_validate's rules and flm_tree_walk, the accept walk's host restatement (csrc/flm_tree.h)."""
import pytest

from fast_llama_amd import capi


@pytest.mark.parametrize("parent,ok", [
    ([-1, 0], True), ([-1, 0, 0, 1, 1, 2], True), ([-1] + list(range(15)), True), ([-1] + [0] * 15, True),       # the smallest, a ragged one, the longest chain, the widest star
    ([-1], False), ([-1] + list(range(16)), False),                                                            # n = 1, n = 17
    ([0, 0, 1], False), ([-1, -1, 0], False),                                                                  # no root, two roots
    ([-1, 2, 1], False), ([-1, 0, 3, 2], False), ([-1, 1], False),                                             # a forward parent, a cycle (2 -> 3 -> 2), a node its own parent
])
def test_tree_validate(parent, ok):
    if ok:
        capi.tree_validate(parent)
    else:
        with pytest.raises(capi.FlmError, match="tree:"):
            capi.tree_validate(parent)


@pytest.mark.parametrize("tokens,parent,a,path", [
    ([5, 7, 7, 9], [-1, 0, 0, 1], [7, 3, 9, 0], [0, 1]),                   # children 1 and 2 hold the same token: the lowest index wins
    ([5, 8, 7, 9, 9], [-1, 0, 0, 2, 2], [7, 0, 9, 4, 4], [0, 2, 3]),       # a non-first sibling, then the lower of two equal children
    ([5, 6, 6], [-1, 0, 0], [4, 6, 6], [0]),                               # nothing accepted
    ([5, 6, 7, 6], [-1, 0, 1, 1], [6, 6, 0, 1], [0, 1, 3]),                # a token that is right under another parent only
])
def test_tree_walk(tokens, parent, a, path):
    assert list(capi.tree_walk(tokens, parent, a)) == path
