"""probe_walk2 over the table's 32-bit slot array (ccj_table_info.slot32, ccj_table_drop_slot32).

Every case asserts table.slot32 before it probes, so none can pass on the 8-byte walk.  The expected
rows, payloads and table positions come from the CPU oracle (its slot array and membership of the
probe keys, L1 + L2), never from the code under test; then the same table is probed again after
drop_slot32() (the 8-byte walk) and must give the same result for every row.  The one-pass split
places a row by atomic reservations, so which chunk a row lands in is free between two calls: the
two runs are compared per original row (row, payload, position), which a per-chunk set comparison
would imply wherever the layouts agree.

Shapes: 8 build keys (32 slots: one 8-slot window per line, the table-end clamp), 2^18 (two
partitions), 2^21 (sixteen: the fixed split's XCD groups, C5's slab order), each against 2^20 probe
keys uniform over twice the build range plus keys whose low word alone matches a build key.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ccj  # noqa: E402

N_PROBE = 1 << 20
INT64_MAX = (1 << 63) - 1


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ccj.device_init(0)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared case arrays are read-only)


def np_murmur(x):
    """hash_functions.h:8-16 on a uint64 array (wrapping multiplies)."""
    x = x.astype(np.uint64)
    c = np.uint64(0xd6e8feb86659fd93)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(32)
        x *= c
        x ^= x >> np.uint64(32)
        x *= c
        x ^= x >> np.uint64(32)
    return x


def build_keys(n_build, seed=3):
    """n_build distinct keys of [0, 2 n_build), shuffled."""
    g = np.random.default_rng(seed)
    return g.permutation(2 * n_build)[:n_build].astype(np.int64)


def probe_keys(build, n_probe=N_PROBE, seed=5):
    """Uniform over twice the build range (hits and misses), then the special keys at fixed rows:
    k + 2^32 and k | 1 << 63 for build keys k (the low word matches, the key does not), 0xFFFFFFFF,
    -1, INT64_MAX, the largest build key and key 0."""
    g = np.random.default_rng(seed)
    rng = 2 * (int(build.max()) + 1)
    pk = g.integers(0, rng, size=n_probe, dtype=np.int64)
    ks = build[:: max(1, len(build) // 16)][:16]
    special = np.concatenate([ks + (1 << 32), ks | np.int64(-(1 << 63)),
                              np.array([0xFFFFFFFF, -1, INT64_MAX, int(build.max()), 0], np.int64)])
    at = 5 + 37 * np.arange(len(special) * 3)  # each special key three times, spread over the first chunks
    pk[at] = np.tile(special, 3)
    return pk, at[:len(special) - 2]  # the rows (first copies) of the keys that are in no table


@functools.lru_cache(maxsize=None)
def case(n_build):
    """(build keys, probe keys, the oracle's answer), computed once per shape and left unchanged:
    hit[i] = probe row i matches, slot[i] = the oracle table's slot of its key (the device table is
    built in the same insertion order)."""
    build = build_keys(n_build)
    pk, never = probe_keys(build)
    ot = O.Table(O.LP, build)
    occ = np.nonzero(ot.table != -1)[0]
    order = np.argsort(ot.table[occ], kind="stable")
    skeys, sslots = ot.table[occ][order], occ[order]
    i = np.clip(np.searchsorted(skeys, pk), 0, len(skeys) - 1)
    hit = skeys[i] == pk
    slot = np.where(hit, sslots[i], -1)
    assert not hit[never].any()  # none of the aliases may match
    rows = np.nonzero(hit)[0].astype(np.uint64)
    want = (len(rows), O.l2_sum(rows, pk[hit]))
    for a in (build, pk, hit, slot):
        a.setflags(write=False)
    return build, pk, ot, hit, slot, want


def per_row(out, chunk, rows):
    """(original row, payload, position or -1) of every match, sorted by row."""
    nc, cap = out["n_chunks"], out["cap"]
    cnt = out["count"][:nc].cpu().numpy().view(np.uint32).astype(np.int64)
    valid = (np.arange(cap)[None, :] < cnt[:, None]).reshape(-1)
    sel = out["sel"].cpu().numpy().view(np.uint32)[:nc * cap][valid].astype(np.int64)
    if not rows:  # chunk-local position -> the split's row map
        base = np.repeat(np.arange(nc, dtype=np.int64) * chunk, cnt)
        sel = out["row_map"].cpu().numpy().view(np.uint32).astype(np.int64)[base + sel]
    pay = out["payload"].cpu().numpy()[:nc * cap][valid]
    pos = (out["pos"].cpu().numpy().view(np.uint32)[:nc * cap][valid].astype(np.int64)
           if out.get("pos") is not None else np.full(len(sel), -1, np.int64))
    o = np.argsort(sel, kind="stable")
    return sel[o], pay[o], pos[o]


def check_exact(out, chunk, rows, pk, hit, slot, want):
    assert int(out["status"].item()) == 0
    got = ccj.result_checksum(out, 0) if rows else \
        ccj.result_checksum(out, chunk, row_map=out["row_map"].to(torch.int64))
    assert got == want  # L1 + L2
    r, pay, pos = per_row(out, chunk, rows)
    assert np.array_equal(r, np.nonzero(hit)[0])  # exactly the matching rows, each once
    assert np.array_equal(pay, pk[r])
    if out.get("pos") is not None:
        assert np.array_equal(pos, slot[r])
    return r, pay, pos


@pytest.mark.parametrize("rows", [True, False])
@pytest.mark.parametrize("chunk", [2048, 1000, 1001])
@pytest.mark.parametrize("n_build", [8, 1 << 18, 1 << 21])
def test_slot32_walk_vs_oracle_and_8_byte_walk(n_build, chunk, rows):
    build, pk, ot, hit, slot, want = case(n_build)
    table = ccj.Table.from_host(ccj.LP, build)
    assert table.slot32 and table.size == ot.size and (n_build != 8 or table.size == 32)
    keys = dev(pk)
    a = check_exact(table.probe_partitioned(keys, chunk, rows=rows), chunk, rows, pk, hit, slot, want)
    table.drop_slot32()
    assert not table.slot32
    b = check_exact(table.probe_partitioned(keys, chunk, rows=rows), chunk, rows, pk, hit, slot, want)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    table.free()


def window_start(h, size):
    """probe_walk2's first 8-slot window of home slot h: never past the table's end or the 32-slot line."""
    s = np.minimum(h, size - 8)
    return np.minimum(s, (s & ~31) + 24)


def test_slot32_long_runs_reach_phase_b():
    """Runs longer than one 8-slot window: some probed keys sit past the first window of their run,
    so their rows go on to phase B (both preconditions asserted; positions checked against the oracle)."""
    build, pk, ot, hit, slot, want = case(1 << 18)
    table = ccj.Table.from_host(ccj.LP, build)
    assert table.slot32
    assert table.max_rounds > 8
    size = ot.size
    home = (np_murmur(pk[hit].astype(np.uint64)) & np.uint64(size - 1)).astype(np.int64)
    past = ((slot[hit] - window_start(home, size)) % size) >= 8
    assert past.any()
    keys = dev(pk)
    check_exact(table.probe_partitioned(keys, 2048, rows=True, pos=True), 2048, True, pk, hit, slot, want)
    table.free()


def test_slot32_c5_payload_columns():
    """C5 on the 16-partition shape (probe_walk2<POS> in slab order + the payload gather): every
    gathered column equals k * (c + 1) + c, positions equal the oracle's slots and the 8-byte run's."""
    build, pk, ot, hit, slot, want = case(1 << 21)
    table = ccj.Table.from_host(ccj.LP, build)
    assert table.slot32
    pay = (build[:, None] * (np.arange(8, dtype=np.int64) + 1)[None, :] + np.arange(8, dtype=np.int64)[None, :])
    table.set_payload(torch.from_numpy(np.ascontiguousarray(pay).reshape(-1)).cuda(), 8)
    keys = dev(pk)
    res = []
    for s32 in (True, False):
        assert table.slot32 == s32
        part = table.alloc_partitioned(len(pk), 2048)
        out = table.alloc_outputs(part["positions"], 2048, rounds=False, payload_cols=8, pos=True)
        out = table.probe_partitioned(keys, 2048, out=out, part=part, rows=True)
        torch.cuda.synchronize()
        res.append(check_exact(out, 2048, True, pk, hit, slot, want))
        nc, cap = out["n_chunks"], out["cap"]
        cnt = out["count"][:nc].cpu().numpy().view(np.uint32).astype(np.int64)
        valid = (np.arange(cap)[None, :] < cnt[:, None]).reshape(-1)
        key = out["payload"].cpu().numpy()[:nc * cap][valid]
        for c in range(8):
            col = out["payload_cols"][c].cpu().numpy()[:nc * cap][valid]
            assert np.array_equal(col, key * (c + 1) + c), c
        table.drop_slot32()
        table.drop_slot32()  # idempotent
    for x, y in zip(*res):
        assert np.array_equal(x, y)
    table.free()


def test_slot32_overflow_route_retries_exact():
    """One key repeated until the split's segments and overflow area fill: FLAG_PART_OVERFLOW, and the
    wrapper's re-run with the exact split walks the 32-bit slots too."""
    build, _, ot, _, _, _ = case(1 << 21)
    table = ccj.Table.from_host(ccj.LP, build)
    assert table.slot32
    g = np.random.default_rng(9)
    pk = g.integers(0, 4 << 21, size=N_PROBE, dtype=np.int64)
    pk[g.random(N_PROBE) < 0.9] = build[12345]
    pk[7] = build[12345] + (1 << 32)
    hit = np.isin(pk, build)
    r = np.nonzero(hit)[0].astype(np.uint64)
    want = (len(r), O.l2_sum(r, pk[hit]))
    keys = dev(pk)
    for s32 in (True, False):
        assert table.slot32 == s32
        out = table.probe_partitioned(keys, 2048, retry=True)
        torch.cuda.synchronize()
        assert int(out["status"].item()) == 0 and out.get("exact_retry")
        assert ccj.result_checksum(out, 2048, row_map=out["row_map"].to(torch.int64)) == want
        table.drop_slot32()
    table.free()


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("special,on", [([0xFFFFFFFE], True), ([0xFFFFFFFF], False), ([-7], False),
                                        ([4242, 4242], False)])
def test_slot32_eligibility(special, on, route):
    """The array exists only for distinct keys in [0, 0xFFFFFFFE]: a largest key of 0xFFFFFFFE keeps it;
    0xFFFFFFFF, one negative key or a duplicated key (max_dup 2) do not.  The probe is exact in all four
    (multiplicities from the oracle's probe)."""
    g = np.random.default_rng(21)
    build = np.concatenate([g.permutation(1 << 13)[:4000].astype(np.int64) + 10000, np.array(special, np.int64)])
    g.shuffle(build)
    table = ccj.Table.from_host(ccj.LP, build) if route == "host" else \
        ccj.Table.on_device(ccj.LP, dev(build))
    assert table.slot32 == on and int(table.max_dup) == len(special)
    pk = g.integers(0, 1 << 15, size=1 << 16, dtype=np.int64)
    sp = np.array(special + [special[0] + (1 << 32), special[0] ^ (1 << 31), 0xFFFFFFFF, 0xFFFFFFFE, -1, INT64_MAX, 0],
                  np.int64)
    pk[3 + 11 * np.arange(len(sp))] = sp
    want = O.Table(O.LP, build).probe_totals(pk, 2048)
    assert want[0] >= len(special) * len(special)
    keys = dev(pk)
    for _ in range(2):
        out = table.probe_partitioned(keys, 2048)
        torch.cuda.synchronize()
        assert int(out["status"].item()) == 0
        assert ccj.result_checksum(out, 2048, row_map=out["row_map"].to(torch.int64)) == want
        table.drop_slot32()  # any table: CCJ_OK
        assert not table.slot32
    table.free()


def test_slot32_reference_build_and_drop():
    """ccj_table_build_reference (both layouts) builds the array too; drop_slot32 is idempotent, clears
    the flag and leaves the probe exact."""
    n_build, n_probe, rng = 1 << 16, 1 << 18, 1 << 17
    want = O.count_uniform(13, 0, n_probe, rng, n_build, 1)
    for layout in (ccj.LAYOUT_DEVICE, ccj.LAYOUT_REFERENCE):
        table = ccj.Table.reference(ccj.LP, n_build, 1, layout)
        assert table.slot32
        assert not ccj.Table.reference(ccj.LP, n_build, 2, layout).slot32  # duplicated keys
        keys = ccj.gen_uniform_keys(n_probe, 13, rng)
        for _ in range(3):
            out = table.probe_partitioned(keys, 2048, rows=True)
            torch.cuda.synchronize()
            assert int(out["status"].item()) == 0 and ccj.result_checksum(out, 0) == want
            table.drop_slot32()
            assert not table.slot32
        table.free()
    chain = ccj.Table.reference(ccj.CHAIN, 1000, 1, ccj.LAYOUT_DEVICE)
    assert not chain.slot32
    chain.drop_slot32()
    chain.free()
