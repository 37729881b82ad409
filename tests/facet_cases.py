"""Facet counts (csrc/facet.hip, csrc/facet_rule.hpp): numpy-only families of (scope table, code columns) and a plain
evaluator with one right answer — np.bincount per (constraint, field) and a sort by (-count, code).  It shares nothing with
the rule header: tests/test_facets.py checks it on written-out cases, tests/test_facets_gpu.py holds the kernels to it.

A case is a dict: scope_ptr i64 [n_cons + 1], rows i64, codes i32 [n_fields, n_rows], n_codes (one int per field), top."""
import numpy as np

T = 2048   # AMDR_FACET_TILE_ROWS: rows of a scope per block of the count pass
B = 4096   # AMDR_FACET_LDS_BINS: the widest field a block bins in LDS
MAX_TOP = 64

LENGTHS = (0, 1, T - 1, T, T + 1, 3 * T + 7)   # no row, one, a tile less one, a tile, a tile and one, four tiles
WIDTHS = (1, B - 1, B, B + 1, 3 * B + 5)       # one value; around the LDS threshold; three windows and a bit
N_ROWS = 4 * T + 3


def evaluate(scope_ptr, rows, codes, n_codes, top):
    """(total i64 [n], missing i64 [n, F], distinct i32 [n, F], code i32 [n, F, top], count i64 [n, F, top]): per
    constraint the rows inside [0, n_rows) are counted — any other row nowhere — by the codes inside [0, n_codes[f]); the
    list is the codes with a count, by count descending and then code ascending, padded with (-1, 0)."""
    scope_ptr, rows = np.asarray(scope_ptr, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    codes = np.atleast_2d(np.asarray(codes, dtype=np.int32))
    n, (nf, n_rows) = scope_ptr.size - 1, codes.shape
    total = np.zeros(n, dtype=np.int64)
    missing = np.zeros((n, nf), dtype=np.int64)
    distinct = np.zeros((n, nf), dtype=np.int32)
    code = np.full((n, nf, top), -1, dtype=np.int32)
    count = np.zeros((n, nf, top), dtype=np.int64)
    for p in range(n):
        r = rows[scope_ptr[p]:scope_ptr[p + 1]]
        r = r[(r >= 0) & (r < n_rows)]
        total[p] = r.size
        for f in range(nf):
            c = codes[f, r].astype(np.int64)
            named = c[(c >= 0) & (c < n_codes[f])]
            missing[p, f] = c.size - named.size
            per = np.bincount(named, minlength=max(int(n_codes[f]), 1))
            have = np.flatnonzero(per)
            distinct[p, f] = have.size
            order = have[np.lexsort((have, -per[have]))][:top]   # the last key is the primary one
            code[p, f, :order.size] = order
            count[p, f, :order.size] = per[order]
    return total, missing, distinct, code, count


def table(lengths, n_rows, rng):
    """Scopes of the given lengths, each a sorted random subset of [0, n_rows)."""
    parts = [np.sort(rng.choice(n_rows, size=int(m), replace=False)).astype(np.int64) for m in lengths]
    scope_ptr = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([p.size for p in parts], out=scope_ptr[1:])
    return scope_ptr, (np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64))


def column(kind, n_codes, n_rows, rng):
    """One code column: "random" (one row in eight without a value), "skewed" (half the rows on one hot code), "same"
    (every row the last code), "distinct" (row r holds code r mod n_codes), "none" (every row -1), "stray" (a third of the
    rows outside [0, n_codes): n_codes itself, a little past it, negative, the i32 limits)."""
    if kind == "same":
        return np.full(n_rows, n_codes - 1, dtype=np.int32)
    if kind == "none" or n_codes == 0:
        return np.full(n_rows, -1, dtype=np.int32)
    if kind == "distinct":
        return (np.arange(n_rows, dtype=np.int64) % n_codes).astype(np.int32)
    c = rng.integers(0, n_codes, size=n_rows).astype(np.int64)
    if kind == "random":
        c[rng.random(n_rows) < 0.125] = -1
    elif kind == "skewed":
        c[rng.random(n_rows) < 0.5] = n_codes // 2
    elif kind == "stray":
        out = rng.random(n_rows) < 1 / 3
        c[out] = rng.choice(np.array([n_codes, n_codes + 3, -5, 2 ** 31 - 1, -2 ** 31], dtype=np.int64), size=int(out.sum()))
    else:
        raise ValueError(kind)
    return c.astype(np.int32)


def case(kinds, n_codes, top, seed, lengths=LENGTHS, n_rows=N_ROWS):
    rng = np.random.default_rng(seed)
    scope_ptr, rows = table(lengths, n_rows, rng)
    codes = np.stack([column(k, int(w), n_rows, rng) for k, w in zip(kinds, n_codes)])
    return {"scope_ptr": scope_ptr, "rows": rows, "codes": np.ascontiguousarray(codes, dtype=np.int32),
            "n_codes": [int(w) for w in n_codes], "top": int(top)}


def ties_case():
    """220 rows, code = row mod 40: codes 0 .. 19 are held by six rows and the rest by five, so with every row in the scope
    a cut at 7 falls among equal counts and the smaller codes must win; the second scope holds rows 0 .. 39, one per code."""
    n_rows = 220
    codes = (np.arange(n_rows) % 40).astype(np.int32)[None, :]
    rows = np.concatenate([np.arange(n_rows), np.arange(40)]).astype(np.int64)
    return {"scope_ptr": np.array([0, n_rows, n_rows + 40], dtype=np.int64), "rows": rows, "codes": codes, "n_codes": [40], "top": 7}


def families():
    """name -> case: the shapes at which the kernels take another path, and the contents that stress a bin."""
    out = {f"width-{w}": case(("random",), (w,), 10, 100 + i) for i, w in enumerate(WIDTHS)}
    out["hot-bin"] = case(("same", "same"), (7, B + 9), 3, 201)            # one bin takes every add: LDS, and global
    out["skewed"] = case(("skewed", "skewed"), (50, 2 * B), 5, 202)
    out["all-distinct"] = case(("distinct",), (N_ROWS,), MAX_TOP, 203)     # every count is 1: the list is the first codes
    out["all-missing"] = case(("none", "none"), (4, 0), 5, 204)
    out["stray-codes"] = case(("stray", "stray"), (6, B + 2), 8, 205)
    out["ties"] = ties_case()
    out["top-1"] = case(("random",), (9,), 1, 206)
    out["top-64"] = case(("random",), (200,), MAX_TOP, 207)
    out["padded"] = case(("random", "random"), (3, 70), MAX_TOP, 208)      # distinct < top: the list ends in padding
    out["three-fields"] = case(("random", "skewed", "stray"), (3, B, 2 * B + 1), 6, 209)
    return out


def many_case(n_cons=70_000, n_rows=997, seed=210):
    """n_cons constraints of one row each: past the 65 535 a grid's y would hold."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_rows, size=n_cons).astype(np.int64)
    codes = np.stack([column("random", 5, n_rows, rng), column("random", B + 1, n_rows, rng)])
    return {"scope_ptr": np.arange(n_cons + 1, dtype=np.int64), "rows": rows, "codes": np.ascontiguousarray(codes, dtype=np.int32),
            "n_codes": [5, B + 1], "top": 2}
