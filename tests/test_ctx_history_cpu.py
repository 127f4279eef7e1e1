"""The tables of tests/ctx_history.py checked on the CPU: the writer table against the entry points of the header, the cells that do not
run and their bound, the geometry of the placements; the catalogue, the Eulerian circuit and its chunks, and that every expectation is
reproducible."""
import collections
import os
import sys

import numpy as np

from cuda_mesh_voxelization_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_history as H  # noqa: E402


# ---- part 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_writer_table_names_every_device_output_of_the_header():
    """a new entry point with a caller-addressed device output cannot be forgotten: the header is parsed, not a list kept by hand"""
    table = {H.writer_function(w) for w in H.WRITERS}
    header = H.header_device_writers()
    assert table == header, (sorted(header - table), sorted(table - header))
    # the parse misses no prototype, whatever it returns: capi.SYMBOLS is the list the export test checks the library against.  (capi's
    # ctypes signatures know no const, so they cannot tell an output from an input; the header can, and every non-const pointer
    # parameter in it is classified by name -- header_device_writers raises on one it does not know.)
    assert set(H.header_prototypes()) == set(capi.SYMBOLS)
    assert table <= set(capi.SYMBOLS)
    # the host forms and vp_multi_* write no caller device memory (host arrays in and out; ctx_history.WRITERS says why) -- by name:
    assert not any(f.endswith("_host") or f.startswith("vp_multi_") for f in table)
    assert len({w.name for w in H.WRITERS}) == len(H.WRITERS)
    # ... and every output parameter of a writer with several has its own row, named after it (the header says which: nothing kept by hand)
    for f, outs in H.header_device_outputs().items():
        rows = [w.name for w in H.WRITERS if H.writer_function(w) == f]
        if len(outs) == 1:                                           # a single output may go without its parameter's name
            rows = [r if ":" in r else "%s:%s" % (f, outs[0]) for r in rows]
        assert sorted(rows) == sorted("%s:%s" % (f, o) for o in outs), (f, outs, rows)
    assert sum(len(o) for o in H.header_device_outputs().values()) == len(H.WRITERS)


def test_placements_are_what_they_are_called():
    for w in H.WRITERS:
        for rec in H.RECORDS:
            nb, rb = H.out_bytes(w, rec), H.range_bytes(rec)
            for p in H.PLACEMENTS:
                want, reason = H.expectation(w, rec, p)
                assert (want == "skip") == (reason is not None)
                if w.kind in ("slot", "free"):
                    continue
                off = H.place(nb, rb, p)
                if off is None:
                    assert p == "inside" and abs(nb - rb) < 32 and want == "skip"
                    continue
                assert nb % 16 == 0 and off % 16 == 0 and -H.PAD <= off and off + nb <= rb + H.PAD, (w.name, rec, p)
                lo, hi = max(off, 0), min(off + nb, rb)                          # the overlap with the range [0, rb)
                if p == "first":
                    assert (lo, hi) == (0, 16)
                elif p == "last":
                    assert (lo, hi) == (rb - 16, rb)
                elif p == "before":
                    assert off + nb == 0
                elif p == "after":
                    assert off == rb
                else:
                    assert (16 <= off and off + nb <= rb - 16) or (off <= -16 and off + nb >= rb + 16)


def test_skipped_cells_are_listed_and_few():
    """more than a tenth of the cells of a writer or of a record skipped fails"""
    skipped = H.skipped_cells()
    for name, rid, p, reason in skipped:                             # (pytest -rP shows the list)
        print("skipped cell: %s x %s, %s: %s" % (name, rid, p, reason))
    per_writer, per_record = collections.Counter(s[0] for s in skipped), collections.Counter(s[1] for s in skipped)
    cells_of_a_writer, cells_of_a_record = len(H.RECORDS) * len(H.PLACEMENTS), len(H.WRITERS) * len(H.PLACEMENTS)
    for w in H.WRITERS:
        assert per_writer[w.name] * 10 <= cells_of_a_writer, (w.name, per_writer[w.name], cells_of_a_writer)
    for rec in H.RECORDS:
        assert per_record[H.rec_id(rec)] * 10 <= cells_of_a_record, (rec, per_record[H.rec_id(rec)], cells_of_a_record)
    # overlaps are refused and neighbours served, but for the calls that replace the vp_jfa_start record themselves
    for w in H.WRITERS:
        for rec in H.RECORDS:
            for p in H.PLACEMENTS:
                want = H.expectation(w, rec, p)[0]
                if want != "skip":
                    restart = w.kind == "restart" and rec.kind.startswith("jfa")
                    assert want == ("refused" if restart or p in ("first", "inside", "last") else "served")


# ---- part 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_catalogue():
    names = [n.name for n in H.CATALOGUE]
    assert len(names) == len(set(names)) == 52
    sides = collections.defaultdict(set)
    for n in H.CATALOGUE:
        sides[n.op].add(n.n)
        assert n.n in (0, 32, 64, 96, 128)
    assert sides.pop("release") == {0}
    for op, s in sides.items():
        assert len(s) >= 2, (op, s)                                  # two sides: context buffers of two sizes
        if op.startswith("meshdist"):
            assert max(s) <= 64
    assert sides["jfa_tiled"] == {64, 96, 128}                       # table kernel; tile kernels from the mask at their smallest side and at a power of two
    want = {"vox_fine_tiled", "vox_d20_tiled", "vox_acc_tiled", "vox_naive", "cvox_tiled", "cvox_naive", "csg", "surface", "jfa_tiled", "jfa_naive",
            "jfa_startrun", "extract", "fill", "morph_dilate", "morph_close", "morph_naive", "edt_border", "edt_sdf_naive", "edt_morph", "comp_label",
            "comp_filter", "surfnets_tiled", "surfnets_naive", "meshdist_tiled", "meshdist_naive"}
    assert set(sides) == want


def test_circuit_has_every_ordered_pair_exactly_once():
    for count in (1, 2, 5, len(H.CATALOGUE)):
        walk = H.euler_circuit(count)
        assert len(walk) == count * count + 1 and walk[0] == walk[-1]
        pairs = collections.Counter(zip(walk, walk[1:]))
        assert len(pairs) == count * count and set(pairs.values()) == {1}
        assert set(pairs) == {(u, v) for u in range(count) for v in range(count)}
    assert H.euler_circuit(len(H.CATALOGUE)) == H.euler_circuit(len(H.CATALOGUE))          # fixed seed
    assert H.euler_circuit(7, 1) != H.euler_circuit(7, 2)


def test_chunks_lose_no_pair():
    walk = H.euler_circuit(len(H.CATALOGUE))
    pieces = H.chunks(walk)
    assert all(2 <= len(p) <= H.CHUNK_CALLS + 1 for p in pieces)
    assert all(a[-1] == b[0] for a, b in zip(pieces, pieces[1:]))
    pairs = [pr for p in pieces for pr in zip(p, p[1:])]
    assert pairs == list(zip(walk, walk[1:]))
    for edges in (1, 2, 299, 300, 301, 600, 601):
        w = list(range(edges + 1))
        assert [pr for p in H.chunks(w) for pr in zip(p, p[1:])] == list(zip(w, w[1:]))


def test_every_expectation_is_reproducible():
    def snapshot():
        out = {}
        for node in H.CATALOGUE:
            dev, host = node.expected()
            out[node.name] = ({k: np.ascontiguousarray(v).tobytes() for k, v in dev.items()}, dict(host),
                              {k: np.ascontiguousarray(v).tobytes() for k, v in node.inputs().items()})
        return out
    H.clear_memo()
    first = snapshot()
    H.clear_memo()
    second = snapshot()
    assert first.keys() == second.keys()
    for name in first:
        assert first[name] == second[name], name
    for name, (dev, host, inputs) in first.items():
        if name != "release_0":
            assert dev and all(len(b) for b in dev.values()), name
