"""cn_linear's tile selection without a device: cn_linear_kernel_name over a grid of descriptors against the names
recorded in tests/golden/linear_tiles.json (choose_linear_tile and linear_mode_bits decide the launch and the name
alike, so a changed entry is a changed launch).

The grid is the full product the cases() loops spell out; its order is the fixture's.  The fixture holds the
result of every case at every M, run-length coded: "names" the distinct kernel names with the epilogue's template
argument (always the descriptor's own) written {epilogue}; "outcomes" the distinct results of a case -- an index
into "names" or the query's negative status, once if every M in "M" gives the same, else a list of one per M;
"runs" pairs (outcome, number of consecutive cases with it).  Regenerate it from a built library with
`python tests/test_linear_tiles.py`.

Not in the grid: mfma_dtype 2 with a_bf16 set (cn_linear rejects it; the name query ignores a_bf16 there)."""
import ctypes
import itertools
import json
import os
import re

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_tiles.json")
FIELDS = ("mfma_dtype", "tile", "a_bf16", "aux0_bf16", "aux12_bf16", "rowv", "K", "ldb", "N", "epilogue", "split")
# both sides of the two-per-CU 128x256 tile's threshold (M > 65,536, the sampler queries' rows) and of 131,072
MS = (1, 1537, 65536, 65537, 131072, 131073, 524288)
# N: 128 and 256 bound the one-tile-spans-every-column tiles; K: 96 (the bf16 ring's depth), 128 (a main loop
# long enough for a one-per-CU epilogue), multiples of 32 that are / are not multiples of 64
NS = (64, 128, 132, 204, 256, 320)
KS = (32, 64, 96, 128, 256, 288)
LDBS = (128, 256)
# (a_bf16, aux0_bf16, aux12_bf16) of the bf16 mode: template mode bits 1, 5, 9, 13
IMAGES = ((0, 0, 0), (1, 0, 0), (0, 1, 1), (1, 1, 0))
MUL = 3
# (epilogue, split); MUL's split output: bit 0 out_split set, bit 1 nsplit < N
EPILOGUES = [(e, s) for e in (0, 1, 2, 3, 4, 5, 6, 8) for s in (range(4) if e == MUL else (0,))]


def cases():
    """Every case of the grid as a tuple in FIELDS order (what rarely changes the selection varies fastest)."""
    for dtype, tile in itertools.product((0, 1, 2), range(5)):
        for img, rowv, k, ldb, n, es in itertools.product(IMAGES if dtype == 1 else IMAGES[:1], (0, 1), KS, LDBS, NS,
                                                          EPILOGUES):
            yield (dtype, tile) + img + (rowv, k, ldb, n) + es


def outcome(case):
    """The kernel name of the case at each M of MS, or the query's negative status."""
    from copenerf import _lib
    f = dict(zip(FIELDS, case))
    d = _lib.LinearDesc()
    d.N, d.K, d.K1, d.ldb = f["N"], f["K"], f["K"], f["ldb"]
    d.mfma_dtype, d.tile, d.epilogue = f["mfma_dtype"], f["tile"], f["epilogue"]
    d.a_bf16, d.aux0_bf16, d.aux12_bf16 = f["a_bf16"], f["aux0_bf16"], f["aux12_bf16"]
    d.nzero = d.nsplit = f["N"]
    # the query reads the pointers as flags only
    d.rowv = d.colv = 16 if f["rowv"] else None
    if f["split"] & 1:
        d.out_split = 16
    if f["split"] & 2:
        d.nsplit = f["N"] - 52
    buf = ctypes.create_string_buffer(256)
    name = _lib.load().cn_linear_kernel_name
    res = []
    for M in MS:
        d.M = M
        n = name(d, buf, 256)
        res.append(buf.value.decode() if n >= 0 else n)
    return res


def record():
    names, outcomes, runs = [], [], []
    for case in cases():
        res = []
        for r in outcome(case):
            if isinstance(r, str):
                # the epilogue is the 8th template argument
                r = re.sub(r"^([^<]*<(?:[^,]*, ){7})%d," % case[FIELDS.index("epilogue")], r"\1{epilogue},", r)
                if r not in names:
                    names.append(r)
                r = names.index(r)
            res.append(r)
        res = res[0] if len(set(res)) == 1 else res
        if res not in outcomes:
            outcomes.append(res)
        if runs and runs[-1][0] == outcomes.index(res):
            runs[-1][1] += 1
        else:
            runs.append([outcomes.index(res), 1])
    return {"fields": list(FIELDS), "M": list(MS), "names": names, "outcomes": outcomes, "runs": runs}


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_is_the_grid():
    fx = load()
    assert tuple(fx["fields"]) == FIELDS and tuple(fx["M"]) == MS
    assert sum(n for _, n in fx["runs"]) == sum(1 for _ in cases())
    assert all(isinstance(o, int) or len(o) == len(MS) for o in fx["outcomes"])


def test_library_reproduces_every_recorded_selection():
    fx = load()
    recorded = itertools.chain.from_iterable([fx["outcomes"][o]] * n for o, n in fx["runs"])
    bad, total = [], 0
    for case, res in zip(cases(), recorded):
        epilogue = case[FIELDS.index("epilogue")]
        for M, got, want in zip(MS, outcome(case), [res] * len(MS) if isinstance(res, int) else res):
            want = fx["names"][want].format(epilogue=epilogue) if want >= 0 else want
            total += 1
            if got != want:
                bad.append((dict(zip(FIELDS, case), M=M), want, got))
    assert not bad, f"{len(bad)} of {total} selections changed, the first: {bad[:3]}"


if __name__ == "__main__":
    import sys
    try:
        import copenerf  # noqa: F401
    except ImportError:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path[:0] = [os.path.join(root, "cope-nerf_amd"), root]
    fx = record()
    runs = [json.dumps(fx["runs"][i:i + 16], separators=(",", ":"))[1:-1] for i in range(0, len(fx["runs"]), 16)]
    with open(FIXTURE, "w") as f:
        f.write('{"fields": %s,\n "M": %s,\n "names": [\n' % (json.dumps(fx["fields"]), json.dumps(fx["M"])))
        f.write(",\n".join(json.dumps(n) for n in fx["names"]) + '\n ],\n "outcomes": ')
        f.write(json.dumps(fx["outcomes"], separators=(",", ":")) + ',\n "runs": [\n')
        f.write(",\n".join(runs) + "\n]}\n")
    print(f"{FIXTURE}: {sum(n for _, n in fx['runs'])} cases x {len(MS)} M in {len(fx['runs'])} runs, "
          f"{len(fx['names'])} names, {os.path.getsize(FIXTURE)} bytes")
