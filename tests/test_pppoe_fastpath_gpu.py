"""PPPoE session-data fast path on the device: pppoe_decap_kernel ahead of
the uplink pipeline, pppoe_encap_kernel behind the downlink pipeline.

Two oracles, both exact (every value is an integer or a byte):

  * metamorphic — a batch of PPPoE session frames must leave the uplink
    exactly as the batch of their IPoE twins does on an identically
    provisioned launcher: verdicts, lengths, bytes and every counter;
  * differential — state, verdict, length, bytes and the eight PPPoE
    counters equal the golden model's on a batch that interleaves every
    frame kind and every REJECT reason, after one launch and after two.

Every row of every batch is compared.  Shapes: batch sizes around the wave
(64) and block (256) edges, and a forced 2-block grid at n = 1061 — three
grid-stride iterations with a ragged tail.  Tables are small and a batch
carries at most one flow per subscriber, so NAT port allocation is
deterministic.  Payloads carry a position-dependent byte pattern, so an
overlapped copy in the wrong order shows.
"""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import DROP, FWD, PASS, TX
from bng_amd.dataplane.packets import (DHCP_DISCOVER, build_dhcp_request,
                                       build_ipv4, ip2u32, ipv4_header)
from bng_amd.pppoe import codec as C

NOW_SEC = 1_700_000_000
NOW_NS = NOW_SEC * 10**9
SERVER_MAC = bytes.fromhex("020000000001")
CORE_MAC = bytes.fromhex("020000000002")
DST = ip2u32("93.184.216.34")
SPOOF_SRC = ip2u32("66.6.6.6")

FORCED_CAP = 2
FORCED_N = FORCED_CAP * 256 * 2 + 37        # 1061
SHAPES = [(1, 0), (63, 0), (64, 0), (65, 0), (257, 0),
          (FORCED_N, FORCED_CAP)]
# IP packet lengths: the bare header first, then every residue mod 16 the
# 16-byte-word copy treats differently
IP_LENS = [20, 32, 33, 36, 39, 40, 41, 47]
assert {x % 16 for x in IP_LENS} == {0, 1, 4, 7, 8, 9, 15}


def shape_id(s):
    return f"n{s[0]}-cap{s[1]}"


def sub_mac(k):
    return (0xAABBCC000000 + k).to_bytes(6, "big")


def sub_ip(k):
    return ip2u32("10.1.0.1") + k


def sub_sid(k):
    return (k * 61 + 1) & 0xFFFF            # distinct for k < 1074


def pattern(n, seed=0):
    return bytes((7 * i + seed) & 0xFF for i in range(n))


def ip_frame(k, ip_len, src=None):
    """IPoE frame of subscriber k whose IP packet is ip_len bytes."""
    src = sub_ip(k) if src is None else src
    if ip_len < 28:                          # bare header, no L4
        return (SERVER_MAC + sub_mac(k) + b"\x08\x00" +
                ipv4_header(src, DST, ip_len - 20, proto=17) +
                pattern(ip_len - 20, k))
    f = build_ipv4(sub_mac(k), SERVER_MAC, src, DST, proto=17,
                   sport=20000 + k, dport=53,
                   payload=pattern(ip_len - 28, k))
    assert len(f) == 14 + ip_len
    return f


def wrap(frame, sid, proto=C.PROTO_IPV4):
    return C.SessionPacket(sid, proto, frame[14:], src_mac=frame[6:12],
                           dst_mac=frame[0:6]).encode()


def twin_len(k):
    return IP_LENS[k % 8] + 16 * ((k // 8) % 3)


def make_gpu(n_subs, pppoe=lambda k: True, has_nat=lambda k: True,
             egress_qos=False):
    from bng_amd.dataplane.launcher import HipLauncher
    return provision(HipLauncher(
        sub_log2=13, sess_log2=13, eim_log2=13, subnat_log2=13, qos_log2=13,
        binding_log2=13, n_pools=16, pppoe_log2=13), n_subs, pppoe, has_nat,
        egress_qos)


def make_cpu(n_subs, pppoe=lambda k: True, has_nat=lambda k: True,
             egress_qos=False):
    from bng_amd.dataplane.launcher import GoldenLauncher
    cpu = GoldenLauncher()
    cpu.dp.now_ns = NOW_NS
    return provision(cpu, n_subs, pppoe, has_nat, egress_qos)


def provision(l, n_subs, pppoe, has_nat, egress_qos):
    l.set_server_config(SERVER_MAC, ip2u32("10.255.255.1"))
    l.add_pool(1, ip2u32("10.1.0.0"), 16, ip2u32("10.1.255.254"),
               ip2u32("8.8.8.8"), ip2u32("1.1.1.1"), 3600)
    l.set_antispoof_config(default_mode=abi.AS_DISABLED, log_violations=True)
    sessions = []
    for k in range(n_subs):
        ip = sub_ip(k)
        l.add_subscriber(sub_mac(k), 1, ip, NOW_SEC + 600)
        if has_nat(k):
            ps = 1024 + (k % 100) * 512
            l.add_subscriber_nat(ip, ip2u32("203.0.113.1") + k // 100,
                                 ps, ps + 511, subscriber_id=k + 1)
        l.set_qos_policy(ip, 0, 0, direction="ingress", now_ns=NOW_NS)
        if egress_qos:
            l.set_qos_policy(ip, 0, 0, direction="egress", now_ns=NOW_NS)
        l.add_binding(sub_mac(k), ipv4=ip, mode=abi.AS_STRICT)
        if pppoe(k):
            sessions.append((sub_sid(k), sub_mac(k), ip, 1492))
    if hasattr(l, "add_pppoe_sessions"):
        l.add_pppoe_sessions(sessions)       # one launch
    else:
        for s in sessions:
            l.add_pppoe_session(*s)
    return l


def all_stats(l):
    return {"dhcp": l.get_stats(), "nat": l.nat_get_stats(),
            "qos": l.qos_get_stats(), "antispoof": l.antispoof_get_stats(),
            "pppoe": l.pppoe_get_stats()}


def lens_of(t):
    return t.cpu().numpy().view(np.uint16).astype(int).tolist()


@pytest.fixture
def grid_cap():
    from bng_amd.dataplane.build import get_ext
    ext = get_ext(required=True)
    try:
        yield ext.set_pkt_grid_cap
    finally:
        ext.set_pkt_grid_cap(0)


# ------------------------------------------------------------ metamorphic
def run_twins(n, stride, frames_a, frames_b, want_state):
    ga, gb = make_gpu(n), make_gpu(n)
    da, la = ga.make_batch(frames_a, stride=stride)
    db, lb = gb.make_batch(frames_b, stride=stride)
    va, oa = ga.uplink(da, la, now_ns=NOW_NS, now_sec=NOW_SEC)
    vb, ob = gb.uplink(db, lb, now_ns=NOW_NS, now_sec=NOW_SEC)
    assert gb.last_pppoe_state.cpu().tolist() == want_state
    assert ga.last_pppoe_state.cpu().tolist() == [abi.PPPOE_NONE] * n
    assert va.cpu().tolist() == vb.cpu().tolist()
    assert lens_of(oa) == lens_of(ob) == [len(f) for f in frames_a]
    assert lens_of(lb) == lens_of(la)        # lens updated in place
    ha, hb = da.cpu().numpy(), db.cpu().numpy()
    for i, f in enumerate(frames_a):
        assert bytes(hb[i, :len(f)]) == bytes(ha[i, :len(f)]), f"row {i}"
    sa, sb = all_stats(ga), all_stats(gb)
    print(sb)
    for grp in ("dhcp", "nat", "qos", "antispoof"):
        assert sa[grp] == sb[grp], grp
    assert sa["pppoe"] == dict.fromkeys(abi.PPPOE_STAT_NAMES, 0)
    assert sb["pppoe"]["decap_ok"] == n and sum(sb["pppoe"].values()) == n
    return va.cpu().tolist(), sb


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_uplink_pppoe_batch_equals_its_ipoe_twins(shape, grid_cap):
    n, cap = shape
    frames_a = [ip_frame(k, twin_len(k)) for k in range(n)]
    frames_b = [wrap(f, sub_sid(k)) for k, f in enumerate(frames_a)]
    # one short PPPoE frame arrives padded to the Ethernet minimum
    assert len(frames_b[0]) == 42
    frames_b[0] = frames_b[0].ljust(60, b"\x00")
    grid_cap(cap)
    v, st = run_twins(n, 512, frames_a, frames_b, [abi.PPPOE_DECAP] * n)
    if n >= 8:
        assert v.count(FWD) >= n // 2
        assert st["nat"]["packets_snat"] > 0


def test_uplink_twins_at_mtu_size_stride_2048():
    lens = [1492, 1491, 1485, 1477, 1476, 20]
    frames_a = [ip_frame(k, L) for k, L in enumerate(lens)]
    frames_b = [wrap(f, sub_sid(k)) for k, f in enumerate(frames_a)]
    assert len(frames_b[0]) == 1514
    v, _ = run_twins(len(lens), 2048, frames_a, frames_b,
                     [abi.PPPOE_DECAP] * len(lens))
    assert v[:5] == [FWD] * 5


# ----------------------------------------------------------- differential
def is_dhcp(f):
    return (len(f) >= 42 and f[12:14] == b"\x08\x00" and f[14] == 0x45 and
            f[23] == 17 and f[36:38] == b"\x00\x43")


def malformed(k, j):
    good = bytearray(wrap(ip_frame(k, 40), sub_sid(k)))
    if j == 0:
        return bytes(good[:21])              # shorter than the headers
    if j == 1:
        good[14] = 0x21                      # version 2
    elif j == 2:
        good[15] = 0xA7                      # a discovery code
    elif j == 3:
        struct.pack_into(">H", good, 18, 1)  # no room for the PPP protocol
    elif j == 4:
        struct.pack_into(">H", good, 18, len(good) - 20 + 1)   # past the end
    else:
        return C.SessionPacket(sub_sid(k), C.PROTO_IPV4, pattern(19, k),
                               src_mac=sub_mac(k),
                               dst_mac=SERVER_MAC).encode()    # IP < 20 B
    return bytes(good)


def mixed_frame(k):
    kind = k % 12
    data = ip_frame(k, twin_len(k))
    if kind == 0:
        return data
    if kind == 1:
        return wrap(data, sub_sid(k))
    if kind == 2:
        return build_dhcp_request(sub_mac(k), DHCP_DISCOVER, xid=0x1000 + k)
    if kind == 3:
        return C.SessionPacket(sub_sid(k), C.PROTO_LCP, C.CPPacket(
            C.ECHO_REQ, k & 0xFF, pattern(4, k)).encode(),
            src_mac=sub_mac(k), dst_mac=SERVER_MAC).encode()
    if kind == 4:
        return SERVER_MAC + sub_mac(k) + b"\x08\x06" + pattern(28, k)
    if kind == 5:                            # session nobody provisioned
        return wrap(data, (sub_sid(k) + 30) & 0xFFFF)
    if kind == 6:                            # right session, foreign MAC
        f = bytearray(wrap(data, sub_sid(k)))
        f[6:12] = sub_mac(k + 1)
        return bytes(f)
    if kind == 7:
        return malformed(k, (k // 12) % 6)
    if kind == 8:                            # padded to the Ethernet minimum
        return wrap(ip_frame(k, 28 + (k // 12) % 8), sub_sid(k)).ljust(
            60, b"\x00")
    if kind == 9:                            # IPCP / PPP IPv6: host's
        proto = C.PROTO_IPCP if (k // 12) % 2 else C.PROTO_IPV6
        return C.SessionPacket(sub_sid(k), proto, pattern(44, k),
                               src_mac=sub_mac(k),
                               dst_mac=SERVER_MAC).encode()
    if kind == 10:                           # spoofed inner source: DROP
        return wrap(ip_frame(k, twin_len(k), src=SPOOF_SRC), sub_sid(k))
    return C.DiscoveryPacket(C.PADI, 0, [(C.TAG_SERVICE_NAME, b"")],
                             src_mac=sub_mac(k)).encode()


def golden_uplink(cpu, frames):
    """HipLauncher.uplink's sequence on the golden model: decap, then the
    fused kernel's dispatch, then REJECT -> DROP.  Returns per frame
    (state, verdict, bytes)."""
    out = []
    for f in frames:
        cpu.dp.now_ns = NOW_NS
        fb = bytearray(f)
        st, L = cpu.dp.pppoe_decap(fb)
        g = bytes(fb[:L]) if st == abi.PPPOE_DECAP else f
        et = struct.unpack_from(">H", g, 12)[0] if len(g) >= 14 else 0
        if et in (0x8863, 0x8864, 0x0806):
            v, res = PASS, g
        elif is_dhcp(g):
            fb = bytearray(g)
            v, n = cpu.dp.dhcp_fastpath(fb)
            res = bytes(fb[:n]) if v == TX else g
        else:
            fb = bytearray(g)
            v = cpu.dp.antispoof(bytes(fb))
            if v == FWD:
                v = cpu.dp.nat44_egress(fb)
            if v == FWD:
                # ingress QoS is keyed by the subscriber's own address
                v = cpu.dp.qos(g, "ingress")
            res = bytes(fb)
        if st == abi.PPPOE_REJECT:
            v = DROP
        out.append((st, v, res))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_decap_kernel_matches_golden(shape, grid_cap):
    n, cap = shape
    frames = [mixed_frame(k) for k in range(n)]
    gpu, cpu = make_gpu(n), make_cpu(n)
    grid_cap(cap)
    for launch in (1, 2):
        data, lens = gpu.make_batch(frames)
        before = data.cpu().numpy().copy()
        state = gpu.pppoe_decap(data, lens).cpu().tolist()
        host, got_len = data.cpu().numpy(), lens_of(lens)
        for i, f in enumerate(frames):
            fb = bytearray(f)
            st, L = cpu.dp.pppoe_decap(fb)
            assert (state[i], got_len[i]) == (st, L), f"row {i}"
            if st == abi.PPPOE_DECAP:
                assert bytes(host[i, :L]) == bytes(fb[:L]), f"row {i}"
            else:                            # untouched over the full stride
                assert (host[i] == before[i]).all(), f"row {i}"
        print(f"launch {launch}: {gpu.pppoe_get_stats()}")
        assert gpu.pppoe_get_stats() == cpu.pppoe_get_stats(), launch
    if n >= 257:
        st = cpu.pppoe_get_stats()
        assert all(st[k] > 0 for k in abi.PPPOE_STAT_NAMES[:5]), st


@pytest.mark.parametrize("sort_by_type", [False, True], ids=["plain", "sort"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_uplink_mixed_batch_matches_golden(shape, sort_by_type, grid_cap):
    n, cap = shape
    frames = [mixed_frame(k) for k in range(n)]
    gpu, cpu = make_gpu(n), make_cpu(n)
    grid_cap(cap)
    for launch in (1, 2):
        # a fresh copy of the frames: replies are built in place
        data, lens = gpu.make_batch(frames)
        before = data.cpu().numpy().copy()
        v, ol = gpu.uplink(data, lens, now_ns=NOW_NS, now_sec=NOW_SEC,
                           sort_by_type=sort_by_type)
        v, ol, ln = v.cpu().tolist(), lens_of(ol), lens_of(lens)
        state = gpu.last_pppoe_state.cpu().tolist()
        host = data.cpu().numpy()
        for i, (st, vd, res) in enumerate(golden_uplink(cpu, frames)):
            assert (state[i], v[i]) == (st, vd), f"row {i} launch {launch}"
            assert ol[i] == len(res), f"row {i}"
            if vd != TX:
                assert ln[i] == len(res), f"row {i}"
            assert bytes(host[i, :len(res)]) == res, f"row {i}"
            if st in (abi.PPPOE_NONE, abi.PPPOE_CTRL, abi.PPPOE_REJECT) \
                    and vd in (PASS, DROP):
                assert (host[i] == before[i]).all(), f"row {i}"
        got, want = all_stats(gpu), all_stats(cpu)
        print(f"launch {launch}: {got}")
        assert got == want, f"counters differ after launch {launch}"
    if n >= 257:
        assert want["dhcp"]["fastpath_hits"] > 0
        assert want["nat"]["packets_snat"] > 0
        assert want["antispoof"]["packets_dropped"] > 0
        assert all(want["pppoe"][k] > 0 for k in abi.PPPOE_STAT_NAMES[:5])


# --------------------------------------------------------------- downlink
def is_pppoe_sub(k):
    return k % 3 != 2


@pytest.mark.parametrize("shape", [(65, 0), (FORCED_N, FORCED_CAP)],
                         ids=shape_id)
def test_downlink_encap_matches_golden(shape, grid_cap):
    n, cap = shape
    gpu = make_gpu(n, pppoe=is_pppoe_sub, egress_qos=True)
    cpu = make_cpu(n, pppoe=is_pppoe_sub, egress_qos=True)
    # uplink first: one flow per subscriber creates the NAT sessions
    twins = [ip_frame(k, 36) for k in range(n)]
    up = [wrap(f, sub_sid(k)) if is_pppoe_sub(k) else f
          for k, f in enumerate(twins)]
    data, lens = gpu.make_batch(up)
    v, _ = gpu.uplink(data, lens, now_ns=NOW_NS, now_sec=NOW_SEC)
    assert v.cpu().tolist() == [FWD] * n
    assert [g[1] for g in golden_uplink(cpu, up)] == [FWD] * n
    host = data.cpu().numpy()
    back = []
    for k in range(n):
        nat_ip = struct.unpack_from(">I", host[k], 26)[0]
        nat_port = struct.unpack_from(">H", host[k], 34)[0]
        back.append(build_ipv4(CORE_MAC, SERVER_MAC, DST, nat_ip, proto=17,
                               sport=53, dport=nat_port,
                               payload=pattern(twin_len(k) - 20, k)))
    grid_cap(cap)
    for launch in (1, 2):
        d2, l2 = gpu.make_batch(back)
        v = gpu.downlink(d2, l2, now_ns=NOW_NS).cpu().tolist()
        state = gpu.last_pppoe_state.cpu().tolist()
        h2, got_len = d2.cpu().numpy(), lens_of(l2)
        for k, f in enumerate(back):
            cpu.dp.now_ns = NOW_NS
            fb = bytearray(f)
            x = cpu.dp.nat44_ingress(fb)
            if x == FWD:
                x = cpu.dp.qos(bytes(fb), "egress")
            twin = bytes(fb)                 # what an IPoE subscriber gets
            st, x, L = cpu.dp.pppoe_encap(fb, x, 512)
            assert (state[k], v[k], got_len[k]) == (st, x, L), f"row {k}"
            assert bytes(h2[k, :L]) == bytes(fb), f"row {k}"
            assert x == FWD
            assert struct.unpack_from(">I", twin, 30)[0] == sub_ip(k)
            if is_pppoe_sub(k):
                assert st == abi.PPPOE_ENCAP and L == len(f) + 8
                p = C.SessionPacket.decode(bytes(h2[k, :L]))
                assert p.session_id == sub_sid(k)
                assert p.ppp_proto == C.PROTO_IPV4
                assert p.dst_mac == sub_mac(k) and p.src_mac == SERVER_MAC
                assert p.payload == twin[14:]
            else:                            # plain subscriber: unchanged
                assert st == abi.PPPOE_NONE and L == len(f)
                assert bytes(h2[k, :L]) == twin
                assert (h2[k, L:] == 0).all()
        got = (gpu.nat_get_stats(), gpu.qos_get_stats(),
               gpu.pppoe_get_stats())
        print(f"launch {launch}: {got}")
        assert got == (cpu.nat_get_stats(), cpu.qos_get_stats(),
                       cpu.pppoe_get_stats())
    n_pppoe = sum(1 for k in range(n) if is_pppoe_sub(k))
    assert cpu.pppoe_get_stats()["encap_ok"] == 2 * n_pppoe


@pytest.mark.parametrize("stride", [512, 2048])
def test_encap_too_big_and_no_room_boundaries(stride):
    """pppoe_encap_kernel alone, every frame already DNAT-ed and FWD (or
    not): the MRU and row-size boundaries, and the rows it must ignore."""
    import torch
    from bng_amd.dataplane.launcher import GoldenLauncher, HipLauncher
    gpu = HipLauncher(sub_log2=13, sess_log2=13, eim_log2=13, subnat_log2=13,
                      qos_log2=13, binding_log2=13, n_pools=16, pppoe_log2=13)
    cpu = GoldenLauncher()
    small, wide = sub_ip(1), sub_ip(2)
    for l in (gpu, cpu):
        l.set_server_config(SERVER_MAC, ip2u32("10.255.255.1"))
        l.add_pppoe_session(0x0001, sub_mac(1), small, mru=100)
        l.add_pppoe_session(0xFFFF, sub_mac(2), wide, mru=4000)

    def to(ip, n):
        f = build_ipv4(CORE_MAC, SERVER_MAC, DST, ip, proto=17, sport=53,
                       dport=4000, payload=pattern(n - 42, n))
        assert len(f) == n
        return f

    cases = [                                # (frame, verdict in, state)
        (to(small, 114), FWD, abi.PPPOE_ENCAP),      # len - 14 == mru
        (to(small, 115), FWD, abi.PPPOE_TOO_BIG),    # len - 14 == mru + 1
        (to(wide, stride - 8), FWD, abi.PPPOE_ENCAP),    # len + 8 == stride
        (to(wide, stride - 7), FWD, abi.PPPOE_NO_ROOM),  # == stride + 1
        (to(wide, stride), FWD, abi.PPPOE_NO_ROOM),
        (to(small, stride - 3), FWD, abi.PPPOE_TOO_BIG),  # MRU checked first
        (to(wide, 42), FWD, abi.PPPOE_ENCAP),
        (to(wide, 43), PASS, abi.PPPOE_NONE),
        (to(wide, 44), DROP, abi.PPPOE_NONE),
        (to(sub_ip(3), 45), FWD, abi.PPPOE_NONE),    # no such subscriber
        (SERVER_MAC + CORE_MAC + b"\x08\x06" + pattern(46), FWD,
         abi.PPPOE_NONE),
        (to(wide, 42)[:33], FWD, abi.PPPOE_NONE),    # too short to hold dst
    ]
    frames = [c[0] for c in cases]
    for launch in (1, 2):
        data, lens = gpu.make_batch(frames, stride=stride)
        before = data.cpu().numpy().copy()
        verdict = torch.tensor([c[1] for c in cases], dtype=torch.uint8,
                               device=gpu.device)
        state = gpu.pppoe_encap(data, lens, verdict).cpu().tolist()
        host, got_len, v = data.cpu().numpy(), lens_of(lens), \
            verdict.cpu().tolist()
        assert state == [c[2] for c in cases]
        for i, (f, vin, _) in enumerate(cases):
            fb = bytearray(f)
            st, vout, L = cpu.dp.pppoe_encap(fb, vin, stride)
            assert (state[i], v[i], got_len[i]) == (st, vout, L), f"row {i}"
            if st == abi.PPPOE_ENCAP:
                assert bytes(host[i, :L]) == bytes(fb), f"row {i}"
            else:
                assert (host[i] == before[i]).all(), f"row {i}"
            if st in (abi.PPPOE_TOO_BIG, abi.PPPOE_NO_ROOM):
                assert vout == PASS
        assert gpu.pppoe_get_stats() == cpu.pppoe_get_stats()
    assert cpu.pppoe_get_stats() == dict(zip(
        abi.PPPOE_STAT_NAMES, [0, 0, 0, 0, 0, 6, 4, 4]))


# -------------------------------------------------------------- lifecycle
def test_session_lifecycle():
    gpu = make_gpu(4, pppoe=lambda k: k < 2)
    assert gpu.pppoe_session_count == 2
    f0 = wrap(ip_frame(0, 40), sub_sid(0))

    def up(frame):
        data, lens = gpu.make_batch([frame])
        v, _ = gpu.uplink(data, lens, now_ns=NOW_NS, now_sec=NOW_SEC)
        return gpu.last_pppoe_state.cpu().tolist()[0], v.cpu().tolist()[0]

    def down(dst_ip):
        f = build_ipv4(CORE_MAC, SERVER_MAC, DST, dst_ip, proto=17, sport=53,
                       dport=9, payload=pattern(10))
        data, lens = gpu.make_batch([f])
        v = gpu.downlink(data, lens, now_ns=NOW_NS)
        return (gpu.last_pppoe_state.cpu().tolist()[0], v.cpu().tolist()[0],
                lens_of(lens)[0] - len(f), bytes(data[0, :6].cpu().numpy()))

    assert up(f0) == (abi.PPPOE_DECAP, FWD)
    assert down(sub_ip(0)) == (abi.PPPOE_ENCAP, FWD, 8, sub_mac(0))

    gpu.remove_pppoe_session(sub_sid(0))
    assert gpu.pppoe_session_count == 1
    assert up(f0) == (abi.PPPOE_REJECT, DROP)
    assert gpu.pppoe_get_stats()["decap_unknown_session"] == 1
    assert down(sub_ip(0))[:3] == (abi.PPPOE_NONE, FWD, 0)

    # the id comes back with subscriber 2's MAC and address
    gpu.add_pppoe_session(sub_sid(0), sub_mac(2), sub_ip(2), mru=1400)
    assert up(f0) == (abi.PPPOE_REJECT, DROP)            # old MAC
    assert gpu.pppoe_get_stats()["decap_mac_mismatch"] == 1
    assert up(wrap(ip_frame(2, 40), sub_sid(0))) == (abi.PPPOE_DECAP, FWD)
    assert down(sub_ip(0))[:3] == (abi.PPPOE_NONE, FWD, 0)   # old address
    assert down(sub_ip(2)) == (abi.PPPOE_ENCAP, FWD, 8, sub_mac(2))

    # re-provisioning a live id with another address drops the stale one
    gpu.add_pppoe_session(sub_sid(0), sub_mac(2), sub_ip(3))
    assert gpu.pppoe_session_count == 2
    assert down(sub_ip(2))[:3] == (abi.PPPOE_NONE, FWD, 0)
    assert down(sub_ip(3)) == (abi.PPPOE_ENCAP, FWD, 8, sub_mac(2))

    # with the last session gone, uplink() and downlink() launch neither
    # kernel: the counters cannot move and PPPoE frames PASS as before
    gpu.remove_pppoe_session(sub_sid(0))
    gpu.remove_pppoe_session(sub_sid(1))
    assert gpu.pppoe_session_count == 0
    before = gpu.pppoe_get_stats()
    gpu.last_pppoe_state = None
    data, lens = gpu.make_batch([f0, ip_frame(1, 40)])
    v, _ = gpu.uplink(data, lens, now_ns=NOW_NS, now_sec=NOW_SEC)
    assert v.cpu().tolist() == [PASS, FWD]
    assert lens_of(lens) == [len(f0), 54]
    d2, l2 = gpu.make_batch([build_ipv4(CORE_MAC, SERVER_MAC, DST, sub_ip(1),
                                        proto=17, sport=53, dport=9)])
    gpu.downlink(d2, l2, now_ns=NOW_NS)
    assert gpu.last_pppoe_state is None
    assert gpu.pppoe_get_stats() == before


# ------------------------------------------------------------------- pump
def test_pump_forwards_with_device_side_lengths():
    """The pump takes forwarded lengths from the device after the call: a
    PPPoE data frame leaves as the same bytes as its IPoE twin (8 shorter
    than it came in), and a return frame leaves 8 longer."""
    from bng_amd.dataplane.pktio import Pump
    twin = ip_frame(0, 47)
    lcp = mixed_frame(3)
    bad = wrap(ip_frame(1, 40), 0x7777)
    seen = []
    a = Pump(make_gpu(2), None, slow_path=seen.append)
    b = Pump(make_gpu(2), None, slow_path=seen.append)
    out_a, _ = a.process([twin])
    out_b, passed = b.process([wrap(twin, sub_sid(0)), lcp, bad])
    assert out_a == out_b and len(out_b) == 1 and len(out_b[0]) == len(twin)
    assert passed == [lcp] and seen == [lcp]
    assert b.stats["fwd"] == 1 and b.stats["passed"] == 1
    assert b.stats["dropped"] == 1
    nat_ip = struct.unpack_from(">I", out_b[0], 26)[0]
    nat_port = struct.unpack_from(">H", out_b[0], 34)[0]
    back = build_ipv4(CORE_MAC, SERVER_MAC, DST, nat_ip, proto=17, sport=53,
                      dport=nat_port, payload=pattern(31))
    down = Pump(b.launcher, None, direction="downlink")
    got, _ = down.process([back])
    assert len(got) == 1 and len(got[0]) == len(back) + 8
    p = C.SessionPacket.decode(got[0])
    assert p.session_id == sub_sid(0) and p.dst_mac == sub_mac(0)
    assert p.payload[28:] == pattern(31)
    assert struct.unpack_from(">I", p.payload, 16)[0] == sub_ip(0)
