"""bench.py --dump-outputs on host tensors (no GPU): the per-row match records of a probe output in
each of the three forms bench.py's paths return (sel relative to the chunk, sel = the row itself,
sel = a position mapped through a row map), and match records with a row outside the probe column
counted instead of indexed."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PROBE, CHUNK = 5000, 256  # a ragged last chunk


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def probe_out():
    """A probe output with a random subset of every chunk's rows matched, payload = 7 * row + 1, one
    payload column = 3 * row; and the expected per-row match count."""
    rng = np.random.default_rng(1)
    n_chunks = (N_PROBE + CHUNK - 1) // CHUNK
    count = np.zeros(n_chunks, np.int32)
    sel = np.zeros(n_chunks * CHUNK, np.int32)
    hit = np.zeros(N_PROBE)
    for c in range(n_chunks):
        live = min(CHUNK, N_PROBE - c * CHUNK)
        s = np.sort(rng.choice(live, rng.integers(0, live + 1), replace=False))
        count[c] = len(s)
        sel[c * CHUNK:c * CHUNK + len(s)] = s
        hit[c * CHUNK + s] = 1
    return dict(count=count, sel=sel, n_chunks=n_chunks, hit=hit)


def as_res(po, sel, row_of_slot):
    """The output dict of ccj.Table.alloc_outputs on the host; row_of_slot: the row behind every slot."""
    pay = np.zeros(len(sel), np.int64)
    col = np.zeros(len(sel), np.int64)
    for c in range(po["n_chunks"]):
        m = po["count"][c]
        r = row_of_slot[c * CHUNK:c * CHUNK + m]
        pay[c * CHUNK:c * CHUNK + m], col[c * CHUNK:c * CHUNK + m] = 7 * r + 1, 3 * r
    return dict(count=torch.from_numpy(po["count"]), sel=torch.from_numpy(sel), payload=torch.from_numpy(pay),
                payload_cols=[torch.from_numpy(col)], n_chunks=po["n_chunks"], cap=CHUNK,
                status=torch.zeros(1, dtype=torch.int32))


def check(bench, tmp_path, res, chunk, row_map, hit):
    names = bench.dump_outputs(str(tmp_path), res, N_PROBE, chunk, row_map)
    assert names == sorted(os.listdir(tmp_path))
    got = {n[:-4]: np.load(tmp_path / n) for n in names}
    assert all(a.dtype == np.float64 for a in got.values())
    rows = got["rows"].astype(np.int64)
    assert np.all(np.diff(rows) > 0) and 0 <= rows[0] and rows[-1] < N_PROBE
    assert np.array_equal(got["match_count"], hit[rows])
    assert np.array_equal(got["payload_sum"], hit[rows] * (7 * rows + 1))
    assert np.array_equal(got["payload_col0_sum"], hit[rows] * (3 * rows))
    assert got["totals"].tolist() == [hit.sum(), 0, 0]
    return got


def test_dump_chunk_relative_sel(bench, probe_out, tmp_path):
    base = np.repeat(np.arange(probe_out["n_chunks"]) * CHUNK, CHUNK)
    a = check(bench, tmp_path, as_res(probe_out, probe_out["sel"], base + probe_out["sel"]), CHUNK, None,
              probe_out["hit"])
    b = bench.dump_outputs(str(tmp_path), as_res(probe_out, probe_out["sel"], base + probe_out["sel"]), N_PROBE, CHUNK)
    assert np.array_equal(a["rows"], np.load(tmp_path / "rows.npy")) and "rows.npy" in b  # the same sample every time


def test_dump_rows_in_sel_and_row_map(bench, probe_out, tmp_path):
    """The partitioned layouts: positions are a permutation of the rows."""
    perm = np.random.default_rng(2).permutation(N_PROBE)
    padded = np.concatenate([perm, np.zeros(probe_out["n_chunks"] * CHUNK - N_PROBE, np.int64)])
    base = np.repeat(np.arange(probe_out["n_chunks"]) * CHUNK, CHUNK)
    row_of_slot = padded[np.minimum(base + probe_out["sel"], len(padded) - 1)]
    hit = np.zeros(N_PROBE)
    hit[perm] = probe_out["hit"]
    check(bench, tmp_path / "rows", as_res(probe_out, row_of_slot.astype(np.int32), row_of_slot), 0, None, hit)
    check(bench, tmp_path / "map", as_res(probe_out, probe_out["sel"], row_of_slot), CHUNK,
          torch.from_numpy(perm.astype(np.int32)), hit)


def test_dump_counts_rows_outside_the_column(bench, probe_out, tmp_path):
    sel = np.where(probe_out["sel"] > 0, probe_out["sel"] + 100000, probe_out["sel"]).astype(np.int32)
    base = np.repeat(np.arange(probe_out["n_chunks"]) * CHUNK, CHUNK)
    bench.dump_outputs(str(tmp_path), as_res(probe_out, sel, base + probe_out["sel"]), N_PROBE, CHUNK)
    total, status, stray = np.load(tmp_path / "totals.npy").tolist()
    live = np.concatenate([sel[c * CHUNK:c * CHUNK + probe_out["count"][c]] for c in range(probe_out["n_chunks"])])
    assert total == probe_out["hit"].sum() and status == 0 and stray == (live >= 100000).sum() > 0
