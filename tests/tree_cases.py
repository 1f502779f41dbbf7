"""Support for the tests of whole search trees (not collected): the invariants that the reference's backup (MCTS._backProp,
MCTS.py:238-258) implies for every edge of a Dynamic-MCTS tree of a strictly alternating two-player game, checked on the rows a
caller can read (bb_node_view / bb_node_edges), from a root all the way down.

For an edge e = (node P, action a) into a child X, with N / W the edge's Plays / Value:
  X expanded:                   N(e) == 1 + sum_b N(X, b)   one visit expanded X, every later one went on through an edge of X
  X neither expanded nor over:  N(e) == 0                   a child made for a move that no simulation tried (advance_root), or a
                                                            leaf that is posted and not applied yet -- so the rule holds wherever a
                                                            persistent launch happens to stop
  X terminal:                   N(e) >= 0, and X has no children
  no node behind e at all:      N(e) == 0 and W(e) == 0
  the root handed in:           root_plays == 1 + sum_b N(root, b)
  values:                       c(X) = W(e) - sum_b (N(X, b) - W(X, b)) is the value term of the ONE visit that expanded X, so
                                0 <= c(X) <= 1: an edge of X and the edge into X receive v and 1 - v of the same simulation
                                (backup_path: pl == prev ? v01 : vflip; the players alternate along a path).
The tolerance of the last rule is derived, not measured (value_tolerance)."""
import numpy as np

from blackbird_amd import _lib

NODE_EXPANDED, NODE_TERMINAL = _lib.NODE_EXPANDED, _lib.NODE_TERMINAL
CHILD_NONE, CHILD_TERM_BIT = _lib.CHILD_NONE, _lib.CHILD_TERM_BIT
U32 = 2.0 ** -24   # unit roundoff of float32


class TreeInvariantError(AssertionError):
    """One broken rule: `node` / `action` name the edge (action None: the root's own rule), `rule` which one."""

    def __init__(self, what, node, action, rule, detail):
        AssertionError.__init__(self, "%s: edge (node %s, action %s): %s: %s" % (what, node, action, rule, detail))
        self.node, self.action, self.rule = node, action, rule


def value_tolerance(n):
    """Bound on |computed c(X) - exact c(X)| for an edge of n visits.  W(e) is a float32 sum of n terms in [0, 1] taken one after
    another: recursive summation errs by at most (n - 1) u sum|x_i| <= (n - 1) n u (u = 2^-24; first order, Higham 4.4).  The
    edges of X hold the other n - 1 visits between them, each W(X, b) summed the same way: together at most (n - 1)^2 u.  Every
    term itself is exact enough: v01 = (v + 1) / 2 and 1 - v01 are single roundings of numbers in [0, 1], u each, n terms on
    either side: 2 n u.  The checker's own arithmetic is float64 on at most 2^24-sized integers and these sums: nothing next
    to that.  Sum: ((n - 1) n + (n - 1)^2 + 2 n) u <= 2 n^2 u + 2 u for n >= 0."""
    return (2.0 * n * n + 2.0) * U32


def child_index(word):
    """Pool index of a child word (the caller has ruled out CHILD_NONE)."""
    return int(word) & ~CHILD_TERM_BIT


def collect_rows(rows, root):
    """Every row of the tree below `root`, the root's first, then level by level in the order of the child words."""
    out, todo = [], [root]
    while todo:
        row, children = rows(todo.pop(0))
        out.append(row)
        todo += [child_index(c) for c in children if c != CHILD_NONE]
    return out


def check_tree(rows, root, root_plays, what=""):
    """rows(node) -> (row, children) as search_cases.view_rows / edge_rows give them for one slot (children[k] goes with
    row['plays'][k] and row['value'][k]); root: the pool index to start from (or -1); root_plays: the root's Plays
    (bb_sample_moves' root_plays).  Walks every node below the root once and raises TreeInvariantError at the first broken
    rule.  Returns dict(nodes, expanded, terminal, pending, depth): how many nodes it saw, of which expanded / terminal /
    neither, and the depth of the deepest."""
    stats = dict(nodes=0, expanded=0, terminal=0, pending=0, depth=0)
    seen = set()

    def fetch(node):
        row, children = rows(node)
        n = np.asarray(row["plays"], dtype=np.int64)[:len(children)]
        w = np.asarray(row["value"], dtype=np.float64)[:len(children)]
        return row, np.asarray(children, dtype=np.int64), n, w

    row, children, n, w = fetch(root)
    me = int(row["node"])
    if not row["flags"] & NODE_EXPANDED:
        if root_plays != 0 or n.any():
            raise TreeInvariantError(what, me, None, "root plays", "a root that is not expanded has plays %d, edges %s" % (root_plays, n))
    elif root_plays != 1 + int(n.sum()):
        raise TreeInvariantError(what, me, None, "root plays", "%d != 1 + %d" % (root_plays, int(n.sum())))
    todo = [(me, row, children, n, w, 0)]
    seen.add(me)
    while todo:
        me, row, children, n, w, depth = todo.pop()
        stats["nodes"] += 1
        stats["depth"] = max(stats["depth"], depth)
        expanded, terminal = bool(row["flags"] & NODE_EXPANDED), bool(row["flags"] & NODE_TERMINAL)
        stats["expanded" if expanded else "terminal" if terminal else "pending"] += 1
        if not expanded:
            if (children >= 0).any() or n.any() or w.any():
                raise TreeInvariantError(what, me, None, "leaf", "a node that is not expanded has children %s plays %s values %s" % (children, n, w))
            continue
        if terminal:
            raise TreeInvariantError(what, me, None, "leaf", "expanded and terminal")
        for a in range(len(children)):
            ne, we = int(n[a]), float(w[a])
            if ne < 0:
                raise TreeInvariantError(what, me, a, "plays", "N = %d" % ne)
            if children[a] == CHILD_NONE:
                if ne != 0 or we != 0.0:
                    raise TreeInvariantError(what, me, a, "no child", "N = %d, W = %r behind no node" % (ne, we))
                continue
            x = child_index(children[a])
            if x in seen:
                raise TreeInvariantError(what, me, a, "tree", "node %d is reached twice" % x)
            seen.add(x)
            xrow, xch, xn, xw = fetch(x)
            if int(xrow["node"]) != x:
                raise TreeInvariantError(what, me, a, "tree", "asked for node %d, got %d" % (x, int(xrow["node"])))
            x_exp, x_term = bool(xrow["flags"] & NODE_EXPANDED), bool(xrow["flags"] & NODE_TERMINAL)
            if bool(int(children[a]) & CHILD_TERM_BIT) != x_term:
                raise TreeInvariantError(what, me, a, "tree", "child word %#x, child flags %#x" % (int(children[a]), xrow["flags"]))
            below = int(xn.sum())
            if x_exp and ne != 1 + below:
                raise TreeInvariantError(what, me, a, "plays", "N = %d != 1 + %d, the plays of node %d's edges" % (ne, below, x))
            if not x_exp and not x_term and ne != 0:
                raise TreeInvariantError(what, me, a, "plays", "N = %d into node %d, which is neither expanded nor terminal" % (ne, x))
            tol = value_tolerance(ne)
            if x_exp:
                c = we - float((xn - xw).sum())
                if not -tol <= c <= 1.0 + tol:
                    raise TreeInvariantError(what, me, a, "value", "c = W - sum(N - W) of node %d = %r outside [0, 1] +- %g" % (x, c, tol))
            elif not -tol <= we <= ne + tol:   # (a terminal child: N values in [0, 1]; a pending one: nothing)
                raise TreeInvariantError(what, me, a, "value", "W = %r of N = %d visits" % (we, ne))
            todo.append((x, xrow, xch, xn, xw, depth + 1))
    return stats
