"""The smallest synthetic structure with a factor launch the deferral pass of the plan dissolves (numpy only), from the
generators of tests/mf_structures.py: a chain of four levels -- nine small leaves (a wide level: one launch per size class)
under a front of 60 x 6, that under 19 x 4, that under the root -- and beside the leaves a front of 56 x 8, the part of the
64-variable clique that touches nothing else: 65 rows with its right-hand-side row, one over the class of four tiles, so
it is alone in a launch of five tiles on level 0 while its parent, the 19 x 4 front, sits on level 2.  The 60 x 6 front on
level 1 runs the same kernel (five tiles, at most eight fronts), and the leaf can ride with it.  At batches up to 64 the
levels merge up to four tiles, which leaves this shape as it is."""
import numpy as np

import mf_structures as MS


def defer_leaf():
    b = MS._Builder(7)
    s = b.clique(64)
    a = b.clique(54); b.couple(a, s[:4]); b.row(np.concatenate([a[:2], s[:1]]), "eq")
    for i in range(9):
        v = b.clique(10); b.couple(v, a[2 * i:2 * i + 2]); b.row(np.concatenate([v[:2], a[2 * i:2 * i + 1]]), "eq")
    f = b.clique(30); b.couple(f, s[4:8]); b.row(np.concatenate([f[:2], s[4:5]]), "eq")
    b.row(s[:3], "eq")
    b.tail()
    return b.done("defer_leaf", {"launches": (5, 4), "moved": (56, 8)})
