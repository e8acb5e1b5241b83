"""The partition of the batched L4 solver (no GPU needed): chip_debug_bplan_create runs the function chip_batch_create
builds its plan with (host_plan_build, csrc/batch.cpp).  Chunks and cone items must cover every index of their space
exactly once, stay inside one member and within BATCH_CHUNK entries, a second-order cone must be one item, and the
per-member ranges and row types must follow from the sizes alone."""
import ctypes as C

import numpy as np
import pytest

from tests import batch_pass_ref as R

ZERO, NN, SOC = R.ZERO, R.NN, R.SOC

PARTITIONS = {"edges": R.part_edges, "cones": R.part_cones, "tiny257": lambda: R.part_tiny(257),
              "tiny600": lambda: R.part_tiny(600), "socs": R.part_socs,
              "nn": lambda: R.part_nn([1, 4096, 0, 4097, 9000]), "zero_only": lambda: ([2, 0, 1], [3, 0, 4097],
                                                                                    [(ZERO, 3), (ZERO, 4097)]),
              "no_rows": lambda: ([0, 5, 0], [0, 0, 0], []), "large": R.part_large}


@pytest.fixture(scope="module", params=sorted(PARTITIONS))
def plan(request, hip):
    n_part, m_part, cones = PARTITIONS[request.param]()
    pl = hip.BatchPlanDebug(n_part, m_part, cones)
    return pl, {k: pl.get(k) for k in pl.NAMES}, n_part, m_part, cones


def test_sizes_and_offsets(plan):
    pl, a, n_part, m_part, cones = plan
    assert (pl.nprob, pl.n, pl.m) == (len(n_part), sum(n_part), sum(m_part))
    assert np.array_equal(a["xoff"], R.offsets(n_part)) and np.array_equal(a["zoff"], R.offsets(m_part))
    assert np.array_equal(a["xmem"], R.members_of(n_part)) and np.array_equal(a["zmem"], R.members_of(m_part))
    assert len(a["ch_beg"]) == len(a["ch_end"]) == pl.ncx + pl.ncz
    assert len(a["it_beg"]) == len(a["it_end"]) == len(a["it_type"]) == pl.nitems
    for name in ("cx_first", "cz_first", "it_first"):
        assert len(a[name]) == pl.nprob + 1, name


def test_chunks_cover_each_space_once_inside_one_member(plan):
    pl, a, n_part, m_part, _ = plan
    for lo, hi, length, mem, first, part in ((0, pl.ncx, pl.n, a["xmem"], a["cx_first"], n_part),
                                             (pl.ncx, pl.ncx + pl.ncz, pl.m, a["zmem"], a["cz_first"], m_part)):
        beg, end = a["ch_beg"][lo:hi].astype(np.int64), a["ch_end"][lo:hi].astype(np.int64)
        assert np.all(end > beg) and np.all(end - beg <= R.CHUNK)  # no empty chunk, none above BATCH_CHUNK
        cover = np.zeros(length + 1, dtype=np.int64)
        np.add.at(cover, beg, 1)
        np.add.at(cover, end, -1)
        assert np.all(np.cumsum(cover)[:length] == 1)  # every index exactly once
        assert np.all(mem[beg] == mem[end - 1])  # a chunk stays inside one member
        # the member's chunks: monotone ranges that hold exactly ceil(size / BATCH_CHUNK) chunks of that member, in
        # entry order
        assert first[0] == 0 and first[-1] == hi - lo and np.all(np.diff(first) >= 0)
        assert np.array_equal(np.diff(first), [-(-int(p) // R.CHUNK) for p in part])
        off = R.offsets(part)
        for k in range(pl.nprob):
            c0, c1 = first[k], first[k + 1]
            if c1 > c0:
                assert beg[c0] == off[k] and end[c1 - 1] == off[k + 1]
                assert np.array_equal(beg[c0 + 1:c1], end[c0:c1 - 1])
                assert np.all(end[c0:c1 - 1] - beg[c0:c1 - 1] == R.CHUNK)  # only the last chunk is short


def test_items_cover_the_cone_rows_once(plan):
    pl, a, _, m_part, cones = plan
    beg, end, typ = a["it_beg"].astype(np.int64), a["it_end"].astype(np.int64), a["it_type"]
    rt = R.row_types(m_part, cones)
    cover = np.zeros(pl.m + 1, dtype=np.int64)
    np.add.at(cover, beg, 1)
    np.add.at(cover, end, -1)
    cover = np.cumsum(cover)[:pl.m]
    assert np.array_equal(cover, (rt != R.ROW_ZERO).astype(np.int64))  # cone rows once, Zero rows never
    assert np.all(end > beg)
    zmem = a["zmem"]
    assert np.all(zmem[beg] == zmem[end - 1])
    nn = typ == R.ITEM_NN
    assert np.all((end - beg)[nn] <= R.CHUNK)
    for b, e, t in zip(beg, end, typ):
        assert np.all(rt[b:e] == R.ROW_NN) if t == R.ITEM_NN else (rt[b] == R.ROW_SOC_HEAD and
                                                                   np.all(rt[b + 1:e] == R.ROW_SOC_TAIL))
    # a second-order cone is exactly one item; a Nonnegative cone ceil(dim / BATCH_CHUNK) items in row order
    want = []
    for tag, r0, r1 in R.cone_ranges(cones):
        if tag == SOC:
            want.append((r0, r1, R.ITEM_SOC))
        elif tag == NN:
            want += [(r, min(r1, r + R.CHUNK), R.ITEM_NN) for r in range(r0, r1, R.CHUNK)]
    assert list(zip(beg.tolist(), end.tolist(), typ.tolist())) == want
    # it_first: the items of member k are [it_first[k], it_first[k + 1])
    first = a["it_first"]
    assert first[0] == 0 and first[-1] == pl.nitems and np.all(np.diff(first) >= 0)
    assert np.array_equal(np.diff(first), np.bincount(zmem[beg], minlength=pl.nprob) if pl.nitems else
                          np.zeros(pl.nprob, dtype=np.int64))
    for k in range(pl.nprob):
        assert np.all(zmem[beg[first[k]:first[k + 1]]] == k)


def test_row_types(plan):
    pl, a, _, m_part, cones = plan
    assert np.array_equal(a["rtype"], R.row_types(m_part, cones))


def test_unknown_name_and_null_arguments(hip):
    pl = hip.BatchPlanDebug([1], [1], [(NN, 1)])
    with pytest.raises(hip.ChipError) as e:
        pl.get("nothing")
    assert e.value.code == hip.ERR_ARG
    L = hip.lib()
    assert L.chip_debug_bplan_get(None, b"xoff", None, None) == hip.ERR_ARG
    assert L.chip_debug_bplan_create(None, C.c_int64(1), None, None, C.c_int64(0), None, None) == hip.ERR_ARG
    L.chip_debug_bplan_destroy(None)


def _rc(hip, n_part, m_part, cones):
    try:
        hip.BatchPlanDebug(n_part, m_part, cones)
    except hip.ChipError as e:
        return e.code
    return 0


def test_refusals_of_parts_and_cones(hip):
    """tests/test_batch_gpu.py::test_refuses_entries_and_cones_across_members, the part of it the plan decides: two
    basic_qp members (2 columns; NN(3), NN(3) rows each)"""
    cones = [(NN, 3)] * 4
    assert _rc(hip, [2, 2], [6, 6], cones) == 0
    assert _rc(hip, [1, 3], [6, 6], cones) == 0  # (columns alone cross nothing: P and A are checked by create itself)
    assert _rc(hip, [2, 2], [4, 8], cones) == hip.ERR_ARG  # the rows split inside the first member's second cone
    assert _rc(hip, [2, 2], [6, 6], [(NN, 3), (NN, 6), (NN, 3)]) == hip.ERR_ARG  # a cone across the boundary
    assert _rc(hip, [2, 2], [6, 5], cones) == hip.ERR_DIM  # the cones do not add up to the rows
    assert _rc(hip, [2, 2], [6, 6], [(SOC, 7), (NN, 5)]) == hip.ERR_ARG  # a second-order cone across the boundary
    assert _rc(hip, [2, -1], [6, 6], cones) == hip.ERR_ARG
    assert _rc(hip, [2, 2], [-6, 18], cones) == hip.ERR_ARG
    assert _rc(hip, [], [], []) == hip.ERR_ARG  # an empty batch
    assert _rc(hip, [2, 2], [6, 6], cones[:3] + [(3, 3)]) == hip.ERR_UNSUPPORTED  # an exponential cone
    assert _rc(hip, [2, 2], [6, 6], cones[:3] + [(6, 2)]) == hip.ERR_UNSUPPORTED  # a PSD cone
    assert _rc(hip, [2 ** 30, 2 ** 30], [0, 0], []) == hip.ERR_DIM  # past int32
    # a cone of no rows at a member boundary belongs to nobody and is accepted, as an empty member is
    assert _rc(hip, [2, 0, 2], [6, 0, 6], [(NN, 3), (NN, 3), (ZERO, 0), (NN, 0), (NN, 6)]) == 0
    # a second-order cone of one row is refused like everywhere in the library, so the passes never meet one
    assert _rc(hip, [1], [1], [(SOC, 1)]) == hip.ERR_ARG
