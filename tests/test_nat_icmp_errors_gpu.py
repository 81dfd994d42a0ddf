"""Inbound ICMP errors through NAT44 (RFC 5508) on the device.

The corpus of `icmp_error_oracle` through `HipLauncher.nat44(egress=False)`
and `downlink()`, after an uplink batch opened the flows: every row first
against the oracle (the error a router would have sent with no NAT on the
path), then byte for byte, verdicts and all counters against the golden
model.  Rows are pre-filled with a sentinel, so a store past a frame shows;
at stride 504 odd rows are not 16-B aligned and take the byte parser.  The
error path writes to no table: the session, reverse, EIM and port-block
tables are compared as raw bytes.
"""
import functools
import random
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import icmp_error_oracle as eo
import wire_oracle as wo
from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import DROP, FWD

NOW_SEC = 1_700_000_000
NOW_NS = NOW_SEC * 10**9
MS = 10**6
SENTINEL = 0xA5
STRIDES = [512, 504]
NEW_STATS = ("icmp_errors_translated", "icmp_errors_unmatched")
FLAGS_ON = abi.NAT_FLAG_EIM | abi.NAT_FLAG_ICMP_ERR


@functools.lru_cache(maxsize=None)
def the_cases():
    return eo.build_cases()


N_ALL = len(the_cases())
SIZES = [1, 64, 65, N_ALL]


def cases_for(n):
    """n cases drawn across the whole corpus, so a short batch holds every
    kind too."""
    cs = the_cases()
    if n == N_ALL:
        return list(cs)
    step = N_ALL // n
    return [cs[(3 + i * step) % N_ALL] for i in range(n)]


# ---------------------------------------------------------------- plumbing
def device_batch(gpu, frames, stride=512):
    """Rows pre-filled with the sentinel past each frame."""
    import torch
    n = len(frames)
    data = np.full((n, stride), SENTINEL, dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint16)
    for i, f in enumerate(frames):
        assert len(f) <= stride
        data[i, :len(f)] = np.frombuffer(f, dtype=np.uint8)
        lens[i] = len(f)
    d = torch.from_numpy(data).to(gpu.device)
    assert d.data_ptr() % 16 == 0
    return d, torch.from_numpy(lens.view(np.int16)).to(gpu.device)


def rows_of(d, lens):
    rows = d.cpu().numpy()
    return [(rows[i, :n].tobytes(), rows[i, n:]) for i, n in enumerate(lens)]


def check_sentinel(i, past):
    assert (past == SENTINEL).all(), (
        f"row {i}: bytes past the frame written at "
        f"{np.nonzero(past != SENTINEL)[0][:8].tolist()} (+len)")


SESSION_DTYPE = [("sig", "<u8"), ("src_ip", "<u4"), ("rest", "116u1")]


def sweep_session_only(gpu, cpu, case):
    """The state a sweep and a reply that has not come yet leave behind:
    the flow's session gone, its reverse entry still there."""
    import torch
    blob = gpu.sessions.cpu().numpy().copy()
    arr = blob.view(SESSION_DTYPE)
    hit = np.nonzero((arr["src_ip"] == case.sub.private_ip) &
                     (arr["sig"] != 0))[0]
    assert len(hit) == 1
    arr["sig"][hit[0]] = 0xFFFFFFFFFFFFFFFF
    gpu.sessions.copy_(torch.from_numpy(blob).to(gpu.device))
    src, dst, proto, sid, did = wo.flow_fields(case.opener)
    del cpu.dp.nat_sessions[(src, dst, sid, 0 if proto == wo.ICMP else did,
                             proto)]


def make_pair(cases, flags=FLAGS_ON, fused=True, **hip_kw):
    """Device and golden launchers with every flow of `cases` open, by one
    uplink batch; what it sent is what the oracle says the NAT sends."""
    from bng_amd.dataplane.launcher import GoldenLauncher, HipLauncher
    cases = eo.Cases(cases)
    cpu = GoldenLauncher()
    cpu.dp.now_ns = NOW_NS
    kw = dict(sub_log2=10, sess_log2=10, eim_log2=10, subnat_log2=10,
              qos_log2=6, binding_log2=10, n_pools=16)
    kw.update(hip_kw)
    gpu = HipLauncher(**kw)
    for l in (gpu, cpu):
        l.set_server_config(wo.GW_MAC, 0x0AFFFF01)
        l.set_antispoof_config(default_mode=abi.AS_DISABLED)
        l.set_nat_config(flags=flags)
        for sub in {c.sub for c in cases}:
            l.add_subscriber_nat(sub.private_ip, sub.public_ip,
                                 sub.port_start, sub.port_end,
                                 subscriber_id=1)
    openers = cases.openers()
    if openers:
        frames = [f for _sub, f in openers]
        d, ln = device_batch(gpu, frames)
        if fused:
            v, _ol = gpu.uplink(d, ln, now_ns=NOW_NS, now_sec=NOW_SEC)
        else:
            v = gpu.nat44(d, ln, egress=True, now_ns=NOW_NS)
        assert v.cpu().tolist() == [FWD] * len(frames)
        for (sub, f), (got, _past) in zip(openers, rows_of(
                d, [len(f) for f in frames])):
            assert got == wo.expected_egress(f, sub.public_ip,
                                             sub.port_start)
            fb = bytearray(f)
            if fused:                        # the uplink kernel's chain
                assert cpu.dp.antispoof(f) == FWD
            assert cpu.dp.nat44_egress(fb) == FWD and bytes(fb) == got
            if fused:
                assert cpu.dp.qos(f, "ingress") == FWD
    for c in cases:
        if c.stale:
            sweep_session_only(gpu, cpu, c)
    assert gpu.nat_get_stats() == cpu.nat_get_stats()
    cpu.dp.now_ns = NOW_NS + MS
    return gpu, cpu


def golden_down(cpu, frame, fused):
    fb = bytearray(frame)
    v = cpu.dp.nat44_ingress(fb)
    if fused and v == FWD:
        v = cpu.dp.qos(bytes(fb), "egress")
    return v, bytes(fb)


def device_down(gpu, frames, stride, fused, order=None, now_ns=NOW_NS + MS):
    """(verdicts, [(frame, bytes past it)]) of one ingress batch."""
    d, ln = device_batch(gpu, frames, stride)
    if fused:
        v = gpu.downlink(d, ln, now_ns=now_ns, order=order)
    else:
        assert order is None
        v = gpu.nat44(d, ln, egress=False, now_ns=now_ns)
    return v.cpu().tolist(), rows_of(d, [len(f) for f in frames])


def nat_tables(gpu):
    """Raw bytes of every table the NAT stage could write to."""
    return tuple(t.cpu().numpy().tobytes()
                 for t in (gpu.sessions, gpu.reverse, gpu.eim, gpu.subctx))


def all_stats(l):
    return {"nat": l.nat_get_stats(), "qos": l.qos_get_stats(),
            "dhcp": l.get_stats(), "antispoof": l.antispoof_get_stats()}


def moved(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def check_rows(cases, v, rows, cpu, fused):
    """Oracle first, then the golden model."""
    for i, (c, (got, past)) in enumerate(zip(cases, rows)):
        where = f"row {i} ({c.name}, len {len(c.err)})"
        assert v[i] == FWD, where
        if c.want == eo.XLATE:
            assert eo.same_error(got, c.expect) == [], where
        else:
            assert eo.untouched(c.err, got) == [], where
        check_sentinel(i, past)
        assert (v[i], got) == golden_down(cpu, c.err, fused), \
            where + ": differs from golden"


def case_id(c):
    return "-".join(str(x) for x in c)


# ============================================================== the corpus
@pytest.mark.parametrize(
    "case", [(n, s, k) for n in SIZES for s in STRIDES
             for k in ("nat44", "downlink")], ids=case_id)
def test_corpus_under_the_oracle(case):
    n, stride, kernel = case
    fused = kernel == "downlink"
    cases = cases_for(n)
    gpu, cpu = make_pair(cases, fused=fused)
    before, tb = all_stats(gpu), nat_tables(gpu)
    v, rows = device_down(gpu, [c.err for c in cases], stride, fused)
    check_rows(cases, v, rows, cpu, fused)
    st = all_stats(gpu)
    assert st == all_stats(cpu)
    want = {"icmp_errors_translated": sum(c.want == eo.XLATE for c in cases),
            "icmp_errors_unmatched": sum(c.want == eo.NOMAP for c in cases)}
    assert moved(before["nat"], st["nat"]) == \
        {k: x for k, x in want.items() if x}
    assert st["qos"] == before["qos"]        # nobody has an egress bucket
    # no-write on the device: last_seen, in-counters, state, stale reverse
    # entries and all
    assert nat_tables(gpu) == tb


@pytest.mark.parametrize("stride", STRIDES)
def test_shuffled_dispatch_order_gives_the_same(stride):
    import torch
    cases = list(the_cases())
    gpu, cpu = make_pair(cases)
    frames = [c.err for c in cases]
    v0, rows0 = device_down(gpu, frames, stride, fused=True)
    st0 = all_stats(gpu)
    order = list(range(len(frames)))
    random.Random(len(frames)).shuffle(order)
    order = torch.from_numpy(np.array(order, dtype=np.int32)).to(gpu.device)
    v1, rows1 = device_down(gpu, frames, stride, fused=True, order=order)
    assert v1 == v0
    assert [r[0] for r in rows1] == [r[0] for r in rows0]
    for i, (_got, past) in enumerate(rows1):
        check_sentinel(i, past)
    check_rows(cases, v1, rows1, cpu, True)
    st1 = all_stats(gpu)
    assert moved(st0["nat"], st1["nat"]) == {
        k: st0["nat"][k] for k in NEW_STATS}


@pytest.mark.parametrize("kernel", ["nat44", "downlink"])
def test_errors_replies_and_strangers_in_one_wave(kernel):
    """Ordinary DNAT hits, errors about the same sessions and unmatched
    errors interleaved lane by lane: the same rows, verdicts, counters and
    tables as one batch per class gives.  The error path leaves the hit
    path alone."""
    fused = kernel == "downlink"
    pos = [c for c in the_cases().by(eo.XLATE)][:64]
    neg = [c for c in the_cases().by(eo.NOMAP) if not c.stale][:64]
    rng = random.Random(11)
    replies = [wo.build_reply(wo.expected_egress(c.opener, c.sub.public_ip,
                                                 c.sub.port_start), rng)
               for c in pos]
    classes = [replies, [c.err for c in pos], [c.err for c in neg]]
    mixed = [f for trio in zip(*classes) for f in trio]
    assert len(mixed) == 192

    gpu, cpu = make_pair(pos + neg, fused=fused)
    v, rows = device_down(gpu, mixed, 512, fused)
    apart, _cpu2 = make_pair(pos + neg, fused=fused)
    va, ra = [], []
    for frames in classes:
        vv, rr = device_down(apart, frames, 512, fused)
        va.append(vv)
        ra.append(rr)
    assert v == [x for trio in zip(*va) for x in trio]
    assert [r[0] for r in rows] == \
        [r[0] for trio in zip(*ra) for r in trio]
    for i, (_got, past) in enumerate(rows):
        check_sentinel(i, past)
    assert all_stats(gpu) == all_stats(apart)
    assert nat_tables(gpu) == nat_tables(apart)
    # and it is the right result: replies reach the subscriber, errors too
    for j, c in enumerate(pos):
        reply, err = rows[3 * j][0], rows[3 * j + 1][0]
        assert wo.verify_frame(reply) == []
        assert struct.unpack_from(">I", reply, 30)[0] == c.sub.private_ip
        assert eo.same_error(err, c.expect) == []
        assert golden_down(cpu, replies[j], fused) == (FWD, reply)
        assert golden_down(cpu, c.err, fused) == (FWD, err)
    for j, c in enumerate(neg):
        assert rows[3 * j + 2][0] == c.err
        assert golden_down(cpu, c.err, fused) == (FWD, c.err)
    st = gpu.nat_get_stats()
    assert st == cpu.nat_get_stats()
    assert (st["packets_dnat"], st["icmp_errors_translated"],
            st["icmp_errors_unmatched"]) == (64, 64, 64)


def test_export_is_equal_before_and_after_errors():
    cases = list(the_cases())
    gpu, _cpu = make_pair(cases)
    before = gpu.export_nat_sessions()
    tb = nat_tables(gpu)
    for fused in (False, True):
        device_down(gpu, [c.err for c in cases], 512, fused,
                    now_ns=NOW_NS + 5 * MS)
    after = gpu.export_nat_sessions()
    assert len(before) == len(after) > 100
    assert before.tobytes() == after.tobytes()
    assert (after["last_seen"] == NOW_NS).all()
    assert nat_tables(gpu) == tb
    arr = np.frombuffer(tb[0], dtype=np.uint64).reshape(-1, 16)
    live = arr[(arr[:, 0] != 0) & (arr[:, 0] != 0xFFFFFFFFFFFFFFFF)]
    assert (live[:, 12] == 0).all()          # packets_in | bytes_in << 24


def test_flag_off_on_the_device():
    cases = list(the_cases())
    for fused in (False, True):
        gpu, cpu = make_pair(cases, flags=abi.NAT_FLAG_EIM, fused=fused)
        before, tb = all_stats(gpu), nat_tables(gpu)
        for stride in STRIDES:
            v, rows = device_down(gpu, [c.err for c in cases], stride, fused)
            assert v == [FWD] * len(cases)
            for i, (c, (got, past)) in enumerate(zip(cases, rows)):
                assert eo.untouched(c.err, got) == [], c.name
                check_sentinel(i, past)
        st = all_stats(gpu)
        assert st["nat"] == before["nat"]
        assert st["nat"]["icmp_errors_translated"] == 0
        assert st["nat"]["icmp_errors_unmatched"] == 0
        assert nat_tables(gpu) == tb
        for c in cases:
            assert golden_down(cpu, c.err, fused) == (FWD, c.err)
        assert cpu.nat_get_stats() == st["nat"]


# ================================================= what follows the DNAT stage
def a_few_errors():
    cs = the_cases()
    return [next(c for c in cs.by(eo.XLATE)
                 if c.name == "plain" and c.opener[23] == p and
                 c.err[34] == t)
            for p, t in ((wo.TCP, 3), (wo.UDP, 11), (wo.ICMP, 12))]


def test_egress_qos_is_keyed_on_the_subscriber():
    """A download bucket of the subscriber with a burst below the frame
    length drops the translated error; one on the public address would
    not have matched anything."""
    cases = a_few_errors()
    gpu, cpu = make_pair(cases)
    tight, roomy, _none = cases
    for l in (gpu, cpu):
        l.set_qos_policy(tight.sub.private_ip, 8000, len(tight.err) - 1,
                         direction="egress", now_ns=NOW_NS + MS)
        l.set_qos_policy(roomy.sub.private_ip, 8000, len(roomy.err),
                         direction="egress", now_ns=NOW_NS + MS)
    v, rows = device_down(gpu, [c.err for c in cases], 512, fused=True)
    assert v == [DROP, FWD, FWD]
    for c, (got, _past), vv in zip(cases, rows, v):
        assert eo.same_error(got, c.expect) == []
        assert golden_down(cpu, c.err, True) == (vv, got)
    assert all_stats(gpu) == all_stats(cpu)
    assert gpu.qos_get_stats()["packets_dropped"] == 1
    assert gpu.nat_get_stats()["icmp_errors_translated"] == 3


def test_accounting_bills_the_private_address():
    cases = a_few_errors()
    gpu, _cpu = make_pair(cases, acct_log2=8)
    ips = [c.sub.private_ip for c in cases]
    gpu.acct_add(ips + [c.sub.public_ip for c in cases[:1]])
    v, _rows = device_down(gpu, [c.err for c in cases], 512, fused=True)
    assert v == [FWD] * 3
    got = gpu.acct_read(ips)
    assert got["down_pkts"].tolist() == [1, 1, 1]
    assert got["down_bytes"].tolist() == [len(c.err) for c in cases]
    assert got["up_pkts"].tolist() == [0, 0, 0]
    pub = gpu.acct_read([cases[0].sub.public_ip])
    assert int(pub["down_pkts"][0]) == 0


def test_pppoe_encap_follows_the_translation():
    cases = a_few_errors()
    gpu, cpu = make_pair(cases)
    for k, c in enumerate(cases):
        for l in (gpu, cpu):
            l.add_pppoe_session(k + 1, c.sub.mac, c.sub.private_ip)
    frames = [c.err for c in cases]
    d, ln = device_batch(gpu, frames, 512)
    v = gpu.downlink(d, ln, now_ns=NOW_NS + MS)
    assert v.cpu().tolist() == [FWD] * 3
    assert gpu.last_pppoe_state.cpu().tolist() == [abi.PPPOE_ENCAP] * 3
    ol = ln.cpu().numpy().view(np.uint16).tolist()
    assert ol == [len(f) + 8 for f in frames]
    for k, (c, (got, past)) in enumerate(zip(cases, rows_of(d, ol))):
        assert got[:6] == c.sub.mac
        assert struct.unpack_from(">HBBHHH", got, 12) == (
            0x8864, 0x11, 0, k + 1, len(c.err) - 14 + 2, 0x0021)
        # behind the session header: the error the oracle wants
        assert eo.same_error(c.expect[:14] + got[22:], c.expect) == []
        check_sentinel(k, past)
        fb = bytearray(c.err)
        assert cpu.dp.nat44_ingress(fb) == FWD
        st, vv, n = cpu.dp.pppoe_encap(fb, FWD, 512)
        assert (st, vv, n, bytes(fb)) == (abi.PPPOE_ENCAP, FWD, ol[k], got)
