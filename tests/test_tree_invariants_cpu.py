"""The tree-invariant checker (tests/tree_cases.py) on hand-built rows, before any GPU is involved: it passes a correct tree and
one caught between the post of a leaf and its backup, and it fails -- naming the edge -- the two trees the defects it is for
would leave behind.

The correct tree (S = 4; the value a simulation brings to the edge INTO the node it reaches, 1 - that to the edge above, ...):
  1  expands the root R = node 0
  2  R -0-> node 1, expanded, 0.75                      3  R -1-> node 2, expanded, 0.25
  4  R -0-> 1 -2-> node 3, expanded, 0.5                 5  R -0-> 1 -2-> 3 -1-> node 4, expanded, 0.125
  6, 7  R -1-> 2 -0-> node 5, terminal, 1.0 both times
  8  R -0-> 1 -2-> 3 -1-> 4 -0-> node 6, expanded, 0.0   (run after the root had moved to node 3: what the chain is for)"""
import copy

import numpy as np
import pytest

from tests import tree_cases as T

S = 4
EXP, TERM = T.NODE_EXPANDED, T.NODE_TERMINAL
NONE, TBIT = T.CHILD_NONE, T.CHILD_TERM_BIT


def _row(node, flags, edges=()):
    """edges: (action, child word, N, W)"""
    r = dict(node=node, flags=flags, child=np.full(S, NONE, np.int32), plays=np.zeros(S, np.int32), value=np.zeros(S, np.float32))
    for a, c, n, w in edges:
        r["child"][a], r["plays"][a], r["value"][a] = c, n, w
    return r


def _correct():
    return {
        0: _row(0, EXP, [(0, 1, 4, 2.375), (1, 2, 3, 0.25)]),
        1: _row(1, EXP, [(2, 3, 3, 1.375)]),
        2: _row(2, EXP, [(0, 5 | TBIT, 2, 2.0)]),
        3: _row(3, EXP, [(1, 4, 2, 1.125)]),
        4: _row(4, EXP, [(0, 6, 1, 0.0)]),
        5: _row(5, TERM),
        6: _row(6, EXP),
    }, 8


def _check(tree, root_plays, root=0):
    def rows(node):
        r = tree[0 if node < 0 else node]   # (-1: the slot's root, as bb_node_view has it)
        return r, r["child"]
    return T.check_tree(rows, root, root_plays, "fixture")


def test_correct_three_ply_tree_passes():
    tree, plays = _correct()
    st = _check(tree, plays)
    assert st == dict(nodes=7, expanded=6, terminal=1, pending=0, depth=4)
    assert _check(tree, plays, root=-1) == st                      # the root by its alias
    assert _check(tree, 3, root=3)["nodes"] == 3                   # and from a node further down, with ITS plays


def test_stale_chain_above_the_current_root_fails_at_its_last_edge():
    """Simulation 8 as the store-only backup leaves it: applied from the then root (node 3) down, the chain's two edges --
    (0, 0) and (1, 2) -- and the top's plays as they were after 7.  The top's rule and the first edge still agree with each other
    (all stale alike); the edge into node 3 does not."""
    tree, _ = _correct()
    tree[0]["plays"][0], tree[0]["value"][0] = 3, 1.375
    tree[1]["plays"][2], tree[1]["value"][2] = 2, 1.375
    with pytest.raises(T.TreeInvariantError) as e:
        _check(tree, 7)
    assert (e.value.node, e.value.action, e.value.rule) == (1, 2, "plays")
    assert "edge (node 1, action 2)" in str(e.value)


def test_plays_bumped_but_value_not_fails_at_that_edge():
    """Simulation 8 counted on edge (0, 0) and its value, 1.0 there, left out: c(node 1) = 1.375 - (3 - 1.375) = -0.25."""
    tree, plays = _correct()
    tree[0]["value"][0] = 1.375
    with pytest.raises(T.TreeInvariantError) as e:
        _check(tree, plays)
    assert (e.value.node, e.value.action, e.value.rule) == (0, 0, "value")
    assert "edge (node 0, action 0)" in str(e.value)


def test_pending_unexpanded_leaf_passes():
    """Between the post of a leaf and its backup: the node exists below edge (6, 3), nothing is counted yet.  The same for a
    child that a move made for an action no simulation had tried."""
    tree, plays = _correct()
    tree = copy.deepcopy(tree)
    tree[6]["child"][3] = 7
    tree[7] = _row(7, 0)
    st = _check(tree, plays)
    assert st["pending"] == 1 and st["nodes"] == 8 and st["depth"] == 5


@pytest.mark.parametrize("case", ["visited_but_not_expanded", "root_plays", "plays_behind_no_node", "terminal_with_children"])
def test_other_broken_trees_fail(case):
    tree, plays = _correct()

    def ninth(action):
        """A ninth simulation down to node 6 and through its edge `action`, value 1.0 there: everything above it consistent."""
        nonlocal plays
        for node, a, v in ((6, action, 1.0), (4, 0, 0.0), (3, 1, 1.0), (1, 2, 0.0), (0, 0, 1.0)):
            tree[node]["plays"][a] += 1
            tree[node]["value"][a] += v
        plays += 1

    if case == "visited_but_not_expanded":
        ninth(3)
        tree[6]["child"][3], tree[7] = 7, _row(7, 0)
        where = (6, 3, "plays")
    elif case == "root_plays":
        plays, where = 7, (0, None, "root plays")
    elif case == "plays_behind_no_node":
        ninth(2)
        where = (6, 2, "no child")
    else:
        tree[5]["child"][0] = 6
        where = (5, None, "leaf")
    with pytest.raises(T.TreeInvariantError) as e:
        _check(tree, plays)
    assert (e.value.node, e.value.action, e.value.rule) == where


def test_value_tolerance_is_far_below_one_skipped_value():
    """The derived bound at the sizes the GPU tests reach (at most a few hundred visits of an edge) against the 0.5 that one
    skipped value moves c by on average."""
    assert T.value_tolerance(0) == 2 * T.U32 and T.value_tolerance(48) < 3e-4 and T.value_tolerance(800) < 0.08
