"""Structures and values for the tests of the dense Newton path (numpy only; nothing from the library).

Built on tests/mf_structures.py.  Each structure is the smallest at which one branch of the dense path is live
(csrc/ipm.hip k_kkt_assemble, solve_vector_at; csrc/order.hip): see the docstring of each builder.  `Case` adds the
two options the dense path reads (kkt_condense, kkt_tile_order) to a structure."""
from __future__ import annotations

import dataclasses

import numpy as np

import mf_structures as MS

B, IDLE = 5, 2                       # instances per context and the one that stays inactive
SENTINEL = -7.5


@dataclasses.dataclass
class Case:
    name: str
    S: MS.Structure
    cond: int = 1
    tile: int = 0
    batch: int = B
    solve: bool = True            # False: assembly and working vector only (the matrix is too large for the numpy LDL^T)
    free_rows: tuple = ()         # rows every instance's values turn ROW_FREE (on top of the random ones)

    @property
    def nu(self):
        return self.S.nu(self.cond)


def _chain_hessian(b, v, rng, extra):
    """a chain along v plus `extra` random couplings inside v: a connected, sparse diagonal block"""
    b.h += [(int(v[i + 1]), int(v[i])) for i in range(len(v) - 1)]
    for _ in range(extra):
        i, j = rng.choice(v, size=2, replace=False)
        b.h.append((int(max(i, j)), int(min(i, j))))


def plain(nu, seed=0):
    """Plain order, condensed: nu = n + 5 unknowns (four equality rows and one inequality row of 33 entries, which the
    length rule keeps), short inequality rows (eliminated).  nu = 63 / 64 / 65: one tile, exactly one, two with 63 padding
    positions; 129: Fpad = 192, a second trip of the 128-thread column loops.  free_rows: the long row (kept and free),
    an equality row (kept and free) and a short inequality row (eliminated and free)."""
    b = MS._Builder(1000 + nu + seed)
    n = nu - 5
    v = b.vars(n)
    _chain_hessian(b, v, b.rng, n // 2)
    for q in range(4):
        b.row(b.rng.choice(v, size=3, replace=False), "eq")
    b.row(b.rng.choice(v, size=33, replace=False), "ineq")            # row 4: kept by its length
    for q in range(12):
        b.row(b.rng.choice(v, size=int(b.rng.integers(1, 6)), replace=False), "ineq")
    S = b.done(f"plain{nu}", {}, kkt_mode=1)
    assert S.nu(1) == nu
    return Case(S.name, S, 1, 0, free_rows=(4, 1, 6))


def full_form(seed=0):
    """Full form (kkt_condense = 0): every row is an unknown of its own, with all three row types."""
    b = MS._Builder(2000 + seed)
    v = b.vars(40)
    _chain_hessian(b, v, b.rng, 25)
    for q in range(8):
        b.row(b.rng.choice(v, size=3, replace=False), "eq")
    for q in range(22):
        b.row(b.rng.choice(v, size=int(b.rng.integers(1, 5)), replace=False), "ineq")
    S = b.done("full70", {}, kkt_mode=1)
    return Case(S.name, S, 0, 0, free_rows=(2, 9, 10))


def tiled(seed=0):
    """Tile order: eight clusters (a sparse connected Hessian block each) around one separator variable.  Per cluster:
    three equality rows of its own (they follow their variables into the leading tile), equality rows that also reach the
    separator (they stay in the remainder), three short inequality rows between the cluster and the separator (eliminated:
    entries between a leading tile and the remainder, and the cliques that make the separator the vertex of highest
    degree).  One equality row on the separator alone touches no leading tile.  Clusters 0 and 1 have 29 variables -- with
    their rows they fill the first leading tile to its last slot -- and twelve rows to the separator; the other six have 24
    variables (two of them leave ten padding slots in a tile) and ten rows: 64 remainder rows touch the first three
    leading tiles, so that with the separator in front exactly one of them starts the second remainder tile."""
    b = MS._Builder(3000 + seed)
    clusters = [b.vars(29 if c < 2 else 24) for c in range(8)]
    s = b.vars(1)
    for v in clusters:
        _chain_hessian(b, v, b.rng, 6)
    for c, v in enumerate(clusters):
        for q in range(3):
            b.row(b.rng.choice(v, size=3, replace=False), "eq")
        for q in range(12 if c < 2 else 10):
            b.row(np.concatenate([b.rng.choice(v, size=2, replace=False), s]), "eq")
        for q in range(3):
            b.row(np.concatenate([b.rng.choice(v, size=2, replace=False), s]), "ineq")
    b.row(s, "eq")
    S = b.done("tiled8x24", {}, kkt_mode=1)
    return Case(S.name, S, 1, 1, free_rows=(0, 5, 16))


def _arrow(noff, hub_diag, tile, seed=0):
    """Arrow Hessian: variable 0 (the hub) coupled to `noff` others, every other variable with its diagonal entry only.
    The hub's column of the full symmetric pattern holds noff + hub_diag entries.  The hub sits in three eliminated
    inequality rows and in an equality row; two more rows stay away from it."""
    b = MS._Builder(4000 + noff + seed)
    b.n = noff + 3
    b.h = [(j, j) for j in range(1, b.n)] + [(j, 0) for j in range(1, noff + 1)]
    if hub_diag:
        b.h.append((0, 0))
    for q in range(3):
        b.row(np.concatenate([[0], b.rng.choice(np.arange(1, b.n), size=3, replace=False)]), "ineq")
    b.row(np.concatenate([[0], b.rng.choice(np.arange(1, b.n), size=2, replace=False)]), "eq")
    b.row(b.rng.choice(np.arange(1, b.n), size=3, replace=False), "eq")
    b.row(b.rng.choice(np.arange(1, b.n), size=4, replace=False), "ineq")
    S = b.done(f"arrow{noff + hub_diag}{'d' if hub_diag else ''}{'_tiled' if tile else ''}", {}, kkt_mode=1)
    return Case(S.name, S, 1, tile, free_rows=(1,))


def _dense_hessian(tile, seed=0):
    """A completely dense Hessian of 260 variables: every column is long (260 entries), some rows of each kind."""
    b = MS._Builder(5000 + seed)
    v = b.clique(260)
    for q in range(3):
        b.row(b.rng.choice(v, size=4, replace=False), "eq")
    for q in range(6):
        b.row(b.rng.choice(v, size=3, replace=False), "ineq")
    S = b.done(f"dense260{'_tiled' if tile else ''}", {}, kkt_mode=1)
    return Case(S.name, S, 1, tile, free_rows=(4,))


def long_columns():
    """The hub column on either side of the `> 256` test of k_kkt_assemble: 256 entries (serial walk), 257 with and 257
    without a diagonal Hessian entry (long-column branch; without: its hdiag stays 0); and the dense Hessian.  Each with
    the tile order off and on (on: the hub is the separator, everything else packs into leading tiles)."""
    out = []
    for tile in (0, 1):
        out += [_arrow(255, True, tile), _arrow(256, True, tile), _arrow(257, False, tile), _dense_hessian(tile)]
    return out


def wide(seed=0):
    """n = 1030, diagonal Hessian, a few rows, plain order: Fpad = 1088 is above the vector kernels' workgroup size, so
    load_solve_vector takes a second trip.  One instance; assembly and working vector only."""
    b = MS._Builder(6000 + seed)
    v = b.vars(1030)
    for q in range(4):
        b.row(b.rng.choice(v, size=3, replace=False), "eq")
    for q in range(8):
        b.row(b.rng.choice(v, size=int(b.rng.integers(2, 6)), replace=False), "ineq")
    S = b.done("wide1030", {}, kkt_mode=1)
    return Case(S.name, S, 1, 0, batch=1, solve=False, free_rows=(5,))


def all_cases():
    return [plain(63), plain(64), plain(65), plain(129), full_form(), tiled()] + long_columns() + [wide()]


CASES = {c.name: c for c in all_cases()}


def values(case: Case, kind: str, seed: int):
    """MS.values with the case's free rows forced: (Jv, Hv, Dd, sigp, hd, rtype, hsc)"""
    Jv, Hv, Dd, sigp, hd, rt, hsc = MS.values(case.S, kind, seed)
    rt = rt.copy()
    rt[list(case.free_rows)] = 0
    return Jv, Hv, Dd, sigp, hd, rt, hsc


def stale_sets(case: Case, seed: int):
    """Value sets A and B of the stale-state test: B turns further rows ROW_FREE, zeroes a third of Jval and has another
    Hessian scale."""
    A = values(case, "well", seed)
    Jv, Hv, Dd, sigp, hd, rt, hsc = values(case, "well", seed + 500)
    rng = np.random.default_rng(seed + 900)
    Jv = np.where(rng.uniform(size=len(Jv)) < 1.0 / 3.0, 0.0, Jv)
    rt = rt.copy()
    rt[rng.uniform(size=len(rt)) < 0.25] = 0
    return A, (Jv, Hv, Dd, sigp, hd, rt, 0.3)
