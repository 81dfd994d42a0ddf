"""NAT44 output of the device under a receiver-side oracle.

Every other GPU test of the NAT rewrite compares the kernel's bytes with
`GoldenDataplane`, a port of the same algorithm.  Here every frame the
device translates is checked by `wire_oracle` directly — checksums summed
from scratch the way the receiving host does, the delta invariant where
that is impossible, `untouched` where NAT must keep its hands off — and
then, additionally, byte for byte against the golden model.

The device has three copies of the rewrite arithmetic: the SNAT
register-window path (16-B aligned row, untagged, ihl 5, 48 bytes or more),
the SNAT byte path and DNAT.  The corpus (wire_oracle.build_corpus) goes
through `nat44` and through `uplink`/`downlink`, at stride 512, where every
row is aligned, and at stride 504, where odd rows are not and take the byte
path; the outputs must agree.  Rows are pre-filled with a sentinel, so a
store past the frame shows.
"""
import functools
import random
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import wire_oracle as wo
from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import FWD, PASS, TX
from bng_amd.dataplane.packets import (DHCP_DISCOVER, DHCP_REQUEST,
                                       build_dhcp_request, ip2u32)

NOW_SEC = 1_700_000_000
NOW_NS = NOW_SEC * 10**9
MS = 10**6
SERVER_MAC = wo.GW_MAC
SERVER_IP = ip2u32("10.255.255.1")
SENTINEL = 0xA5

WANT_VERDICT = {wo.SCRATCH: FWD, wo.DELTA: FWD, wo.UNTOUCHED_FWD: FWD,
                wo.UNTOUCHED_PASS: PASS}


@functools.lru_cache(maxsize=None)
def the_corpus():
    return wo.build_corpus()


N_ALL = len(the_corpus().entries)
SIZES = [1, 64, 65, N_ALL]
STRIDES = [512, 504]


def entries_for(n):
    """n entries; the short batches are drawn across the whole corpus, so
    they hold every kind of frame too."""
    ent = the_corpus().entries
    if n == N_ALL:
        return list(ent)
    step = N_ALL // n
    return [ent[(5 + i * step) % N_ALL] for i in range(n)]


# ---------------------------------------------------------------- plumbing
def configure(l, entries):
    l.set_server_config(SERVER_MAC, SERVER_IP)
    l.add_pool(1, ip2u32("10.1.0.0"), 16, ip2u32("10.1.255.254"),
               ip2u32("8.8.8.8"), ip2u32("1.1.1.1"), 3600)
    l.set_antispoof_config(default_mode=abi.AS_DISABLED, log_violations=True)
    for e in entries:
        s = e.sub
        l.add_subscriber_nat(s.private_ip, s.public_ip, s.port_start,
                             s.port_end, subscriber_id=1)
    return l


def make_pair(entries):
    from bng_amd.dataplane.launcher import GoldenLauncher, HipLauncher
    cpu = GoldenLauncher()
    cpu.dp.now_ns = NOW_NS
    gpu = HipLauncher(sub_log2=10, sess_log2=10, eim_log2=10, subnat_log2=10,
                      qos_log2=6, binding_log2=10, n_pools=16)
    return configure(gpu, entries), configure(cpu, entries)


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


def shuffled_order(gpu, n):
    import torch
    order = list(range(n))
    random.Random(n).shuffle(order)
    return torch.from_numpy(np.array(order, dtype=np.int32)).to(gpu.device)


def all_stats(l):
    return {"dhcp": l.get_stats(), "nat": l.nat_get_stats(),
            "qos": l.qos_get_stats(), "antispoof": l.antispoof_get_stats()}


def golden_up(cpu, frame, fused):
    """(verdict, bytes) of the golden model; fused = the uplink kernel's
    chain (antispoof, SNAT, ingress QoS), else SNAT alone."""
    fb = bytearray(frame)
    if not fused:
        return cpu.dp.nat44_egress(fb), bytes(fb)
    v = cpu.dp.antispoof(bytes(fb))
    if v == FWD:
        v = cpu.dp.nat44_egress(fb)
        if v == FWD:
            v = cpu.dp.qos(bytes(frame), "ingress")
    return v, bytes(fb)


def golden_down(cpu, frame, fused):
    fb = bytearray(frame)
    v = cpu.dp.nat44_ingress(fb)
    if fused and v == FWD:
        v = cpu.dp.qos(bytes(fb), "egress")
    return v, bytes(fb)


def rows_of(d, lens):
    """[(frame bytes, bytes past the frame)] of a device batch."""
    rows = d.cpu().numpy()
    return [(rows[i, :n].tobytes(), rows[i, n:]) for i, n in enumerate(lens)]


def check_sentinel(i, past):
    assert (past == SENTINEL).all(), (
        f"row {i}: bytes past the frame written at "
        f"{np.nonzero(past != SENTINEL)[0][:8].tolist()} (+len)")


def run_egress(gpu, cpu, entries, stride, fused, ordered=False):
    """The entries through SNAT; every row under the oracle, then against
    the golden model.  Returns the device's output frames."""
    frames = [e.frame for e in entries]
    d, l = device_batch(gpu, frames, stride)
    if fused:
        order = shuffled_order(gpu, len(frames)) if ordered else None
        v, ol = gpu.uplink(d, l, now_ns=NOW_NS, now_sec=NOW_SEC, order=order)
        assert ol.cpu().numpy().view(np.uint16).tolist() == \
            [len(f) for f in frames]
    else:
        v = gpu.nat44(d, l, egress=True, now_ns=NOW_NS)
    v = v.cpu().tolist()
    out = []
    for i, (e, (got, past)) in enumerate(zip(entries, rows_of(
            d, [len(f) for f in frames]))):
        where = f"row {i} ({e.cls}, len {len(e.frame)})"
        assert wo.audit_egress(e, got) == [], where
        assert v[i] == WANT_VERDICT[e.check], where
        check_sentinel(i, past)
        wv, wb = golden_up(cpu, e.frame, fused)
        assert (v[i], got) == (wv, wb), where + ": differs from golden"
        out.append(got)
    return out


def run_ingress(gpu, cpu, entries, translated, stride, fused):
    replies = wo.build_replies(entries, translated)
    frames = [r for _i, r in replies]
    d, l = device_batch(gpu, frames, stride)
    if fused:
        v = gpu.downlink(d, l, now_ns=NOW_NS + MS)
    else:
        v = gpu.nat44(d, l, egress=False, now_ns=NOW_NS + MS)
    cpu.dp.now_ns = NOW_NS + MS
    assert v.cpu().tolist() == [FWD] * len(frames)
    for j, ((i, reply), (got, past)) in enumerate(zip(replies, rows_of(
            d, [len(f) for f in frames]))):
        where = f"reply {j} to row {i} ({entries[i].cls}, len {len(reply)})"
        assert wo.verify_frame(reply) == [], where
        assert wo.audit_ingress(entries[i], reply, got) == [], where
        check_sentinel(j, past)
        assert (FWD, got) == golden_down(cpu, reply, fused), \
            where + ": differs from golden"
    cpu.dp.now_ns = NOW_NS
    return len(frames)


def case_id(c):
    return "-".join(str(x) for x in c)


# =========================================================== stand-alone NAT
@pytest.mark.parametrize("case", [(n, s) for n in SIZES for s in STRIDES],
                         ids=case_id)
def test_nat44_kernel_under_the_oracle(case):
    n, stride = case
    entries = entries_for(n)
    gpu, cpu = make_pair(entries)
    out = run_egress(gpu, cpu, entries, stride, fused=False)
    assert gpu.nat_get_stats() == cpu.nat_get_stats()
    n_replies = run_ingress(gpu, cpu, entries, out, stride, fused=False)
    st = gpu.nat_get_stats()
    assert st == cpu.nat_get_stats()
    assert st["packets_snat"] == st["packets_dnat"] == n_replies
    assert st["packets_passed"] == sum(
        e.check == wo.UNTOUCHED_PASS for e in entries)


# ============================================================ fused pipelines
UPLINK_CASES = [(n, s, "plain") for n in SIZES for s in STRIDES] + \
               [(n, s, "order") for n in (65, N_ALL) for s in STRIDES]


@pytest.mark.parametrize("case", UPLINK_CASES, ids=case_id)
def test_uplink_then_downlink_under_the_oracle(case):
    n, stride, order = case
    entries = entries_for(n)
    gpu, cpu = make_pair(entries)
    out = run_egress(gpu, cpu, entries, stride, fused=True,
                     ordered=order == "order")
    assert all_stats(gpu) == all_stats(cpu)
    n_replies = run_ingress(gpu, cpu, entries, out, stride, fused=True)
    assert all_stats(gpu) == all_stats(cpu)
    assert gpu.nat_get_stats()["packets_dnat"] == n_replies


def test_layouts_and_entry_points_agree():
    """One frame, four ways to the device — aligned or not, stand-alone
    kernel or fused pipeline: the same bytes.  At stride 504 the odd rows
    are misaligned; the corpus shifted by one row puts every frame on an
    odd row once, so each frame meets both SNAT rewriters."""
    entries = list(the_corpus().entries)
    outs = {}
    for stride in STRIDES:
        for fused in (False, True):
            for shift in (0, 1):
                ent = entries[-1:] + entries[:-1] if shift else entries
                gpu, cpu = make_pair(ent)
                out = run_egress(gpu, cpu, ent, stride, fused)
                outs[stride, fused, shift] = out[1:] + out[:1] if shift \
                    else out
    first = outs[512, False, 0]
    assert sum(a != e.frame for a, e in zip(first, entries)) > 200
    for key, out in outs.items():
        assert out == first, key
    # the register path was eligible: aligned rows with untagged ihl-5
    # frames of 48 bytes or more, of each protocol, were translated
    for proto in (wo.TCP, wo.UDP, wo.ICMP):
        assert any(e.check == wo.SCRATCH and len(e.frame) >= 48 and
                   e.frame[14] == 0x45 and e.frame[23] == proto
                   for e in entries[1::2])


# ======================================= what NAT must keep its hands off
def test_malformed_fragment_and_icmp_error_classes():
    """bad_ihl, bad_version: not IPv4, FWD, every stage leaves them alone.
    frag_nonfirst, icmp_error: PASS to the host from a NATed subscriber,
    counted as passed; FWD from anyone else.  short_l4: FWD.  On ingress
    all of them: FWD, untouched, no counter moved — with sessions live
    whose tuples their bytes would match if read as ports."""
    corpus = the_corpus()
    ent = [e for e in corpus.entries
           if e.check in (wo.UNTOUCHED_FWD, wo.UNTOUCHED_PASS)]
    live = [e for e in corpus.entries if e.cls == "payload_len"]
    cl = {c: sum(e.cls == c for e in ent) for c in
          ("bad_ihl", "bad_version", "frag_nonfirst", "icmp_error",
           "short_l4")}
    assert all(cl.values()) and sum(cl.values()) == len(ent)
    n_pass = cl["frag_nonfirst"] + cl["icmp_error"]
    for fused in (False, True):
        for stride in STRIDES:
            gpu, cpu = make_pair(ent + live)
            run_egress(gpu, cpu, live, stride, fused)
            before = gpu.nat_get_stats()
            out = run_egress(gpu, cpu, ent, stride, fused)
            assert out == [e.frame for e in ent]
            st = gpu.nat_get_stats()
            assert st == cpu.nat_get_stats()
            moved = {k: st[k] - before[k] for k in st if st[k] != before[k]}
            assert moved == {"packets_passed": n_pass}
            # no session, no port: every block of theirs is still fresh
            assert st["sessions_created"] == len(live)
            # ingress
            frames = [e.frame for e in ent]
            d, l = device_batch(gpu, frames, stride)
            v = gpu.downlink(d, l, now_ns=NOW_NS) if fused else \
                gpu.nat44(d, l, egress=False, now_ns=NOW_NS)
            assert v.cpu().tolist() == [FWD] * len(ent)
            for i, (got, past) in enumerate(rows_of(
                    d, [len(f) for f in frames])):
                assert wo.untouched(frames[i], got) == [], ent[i].cls
                check_sentinel(i, past)
            for f in frames:
                assert golden_down(cpu, f, fused) == (FWD, f)
            assert gpu.nat_get_stats() == cpu.nat_get_stats() == st
    # the same frames from a private source nobody gave a NAT context, and
    # from a public one
    gpu, cpu = make_pair([])
    frames = [e.frame for e in ent]
    public = [f[:26] + b"\x08\x08\x04\x04" + f[30:] for f in frames]
    for batch, want in ((frames, None), (public, FWD)):
        d, l = device_batch(gpu, batch)
        v = gpu.nat44(d, l, egress=True, now_ns=NOW_NS).cpu().tolist()
        gold = [golden_up(cpu, f, False) for f in batch]
        assert v == [g[0] for g in gold]
        assert want is None or v == [want] * len(batch)
        assert [r[0] for r in rows_of(d, [len(f) for f in batch])] == batch
        assert gpu.nat_get_stats() == cpu.nat_get_stats()


# ===================================================================== PPPoE
def pppoe_wrap(frame, sid):
    ip = frame[14:]
    return frame[:12] + struct.pack(">HBBHHH", 0x8864, 0x11, 0, sid,
                                    len(ip) + 2, 0x0021) + ip


def test_pppoe_session_data_decap_then_snat(stride=512):
    """ihl-5 corpus frames wrapped as PPPoE session data: after the decap
    and SNAT they verify from scratch and equal what the same frames give
    as IPoE.  (The PPPoE fast path takes strides that are multiples of 16
    only, so every row is aligned.)"""
    ent = [e for e in the_corpus().entries
           if e.check == wo.SCRATCH and e.frame[14] == 0x45][:96]
    assert {e.frame[23] for e in ent} == {wo.TCP, wo.UDP, wo.ICMP}
    gpu, cpu = make_pair(ent)
    for k, e in enumerate(ent):
        gpu.add_pppoe_session(k + 1, e.sub.mac, e.sub.private_ip)
    frames = [pppoe_wrap(e.frame, k + 1) for k, e in enumerate(ent)]
    d, l = device_batch(gpu, frames, stride)
    v, ol = gpu.uplink(d, l, now_ns=NOW_NS, now_sec=NOW_SEC)
    assert gpu.last_pppoe_state.cpu().tolist() == [abi.PPPOE_DECAP] * len(ent)
    assert v.cpu().tolist() == [FWD] * len(ent)
    ol = ol.cpu().numpy().view(np.uint16).tolist()
    assert ol == [len(e.frame) for e in ent]
    rows = d.cpu().numpy()
    for i, e in enumerate(ent):
        got = rows[i, :ol[i]].tobytes()
        assert wo.audit_egress(e, got) == [], (i, e.cls)
        assert wo.verify_frame(got) == []
        assert (FWD, got) == golden_up(cpu, e.frame, True), (i, e.cls)
        # the decap moves the packet down 8 bytes and leaves the tail of
        # the longer PPPoE frame behind; past that, the sentinel
        check_sentinel(i, rows[i, len(frames[i]):])
    assert gpu.nat_get_stats() == cpu.nat_get_stats()


# ================================================================ DHCP replies
def test_dhcp_replies_are_valid_on_the_wire():
    """TX replies of one small mixed batch: the IP header verifies from
    scratch, the UDP checksum is 0 (none), UDP length and IP total length
    agree with out_len, tags included."""
    entries = entries_for(8)
    gpu, _cpu = make_pair(entries)
    macs = [(0xAABBCC000000 + k).to_bytes(6, "big") for k in range(6)]
    for k, mac in enumerate(macs):
        gpu.add_subscriber(mac, 1, ip2u32("10.1.0.1") + k, NOW_SEC + 600)
    gpu.add_vlan_subscriber(100, 0, 1, ip2u32("10.1.9.2"), NOW_SEC + 600)
    gpu.add_vlan_subscriber(200, 30, 1, ip2u32("10.1.9.3"), NOW_SEC + 600)
    reqs = [
        (0, build_dhcp_request(macs[0], DHCP_DISCOVER, xid=1)),
        (0, build_dhcp_request(macs[1], DHCP_REQUEST, xid=2, broadcast=True)),
        (0, build_dhcp_request(macs[2], DHCP_REQUEST, xid=3,
                               ciaddr=ip2u32("10.1.0.3"))),
        (0, build_dhcp_request(macs[3], DHCP_DISCOVER, xid=4,
                               giaddr=ip2u32("10.9.0.1"))),
        (0, build_dhcp_request(macs[4], DHCP_DISCOVER, xid=5,
                               pad_before_53=3)),
        (4, build_dhcp_request(macs[5], DHCP_DISCOVER, xid=6, c_tag=100)),
        (8, build_dhcp_request(macs[5], DHCP_REQUEST, xid=7, s_tag=200,
                               c_tag=30)),
    ]
    frames, tags = [], []
    for k, e in enumerate(entries):             # interleaved with data
        frames.append(e.frame)
        tags.append(None)
        if k < len(reqs):
            frames.append(reqs[k][1])
            tags.append(reqs[k][0])
    for stride in STRIDES:
        d, l = device_batch(gpu, frames, stride)
        v, ol = gpu.uplink(d, l, now_ns=NOW_NS + stride, now_sec=NOW_SEC)
        v = v.cpu().tolist()
        ol = ol.cpu().numpy().view(np.uint16).tolist()
        rows = d.cpu().numpy()
        for i, tag in enumerate(tags):
            if tag is None:
                assert v[i] != TX
                continue
            assert v[i] == TX, i
            reply = rows[i, :ol[i]].tobytes()
            ip = reply[:12] + reply[12 + tag:]          # tags stripped
            lay = wo.layout(ip)
            assert not isinstance(lay, str), lay
            assert wo.verify_frame(ip) == [], i
            assert lay.proto == wo.UDP and lay.ihl == 20
            assert lay.total == len(ip) - 14
            assert struct.unpack_from(">H", ip, 38)[0] == lay.total - 20
            assert struct.unpack_from(">H", ip, 40)[0] == 0
            m = max(ol[i], len(frames[i]))
            check_sentinel(i, rows[i, m:])
