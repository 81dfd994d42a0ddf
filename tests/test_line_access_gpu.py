"""How the packet kernels touch a line must not show in what they compute.

The fused uplink kernel reads each packet header once into a register
window and serves the ethertype pre-check, the antispoof stage and the spoof
log from it; binding and subscriber-context fields travel by value from the
probe that matched their key (rate and burst fetched right behind it); the
classifier decides from three 8-B words without running the parser.
Every case here goes through `launcher.uplink` and is compared with
`GoldenDataplane`: verdict, out_len, every byte of every row up to the
stride, the four counter groups, the session table and the spoof ring.

Shapes: n = 1, 63, 64, 65 and 257 on a grid capped at two blocks, with and
without an `order` array.  Two blocks hold 512 threads, so those shapes are
one loop iteration each; n = 257 on a ONE-block grid is added, two
iterations, the second one partial.

The helpers (launcher pair, batch upload, row comparison) are those of
test_uplink_snapshots_gpu.
"""
import functools
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_uplink_snapshots_gpu as snap
from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import DROP, GoldenDataplane
from bng_amd.dataplane.packets import (DHCP_DISCOVER, DHCP_REQUEST,
                                       build_dhcp_request, build_ipv4, ip2u32)

NOW_NS, MS = snap.NOW_NS, snap.MS
SERVER_MAC, DST, SPOOF_SRC = snap.SERVER_MAC, snap.DST, snap.SPOOF_SRC
sub_mac, sub_ip = snap.sub_mac, snap.sub_ip

# (n, grid cap in blocks, order array)
SHAPES = [(1, 2, False), (63, 2, True), (64, 2, False), (65, 2, True),
          (257, 2, False), (257, 2, True), (257, 1, True)]


def shape_id(s):
    return f"n{s[0]}-cap{s[1]}-{'order' if s[2] else 'plain'}"


@pytest.fixture
def grid_cap():
    """Setter for the packet-kernel grid cap; always restored to default."""
    from bng_amd.dataplane.build import get_ext
    ext = get_ext(required=True)
    try:
        yield ext.set_pkt_grid_cap
    finally:
        ext.set_pkt_grid_cap(0)


# ------------------------------------------------------------ classification
def golden_class(f):
    """1 when GoldenDataplane.dhcp_fastpath takes the frame for UDP to port
    67 (its header walk, golden.py), else 0."""
    n = len(f)
    if n < 14:
        return 0
    proto, off = struct.unpack_from(">H", f, 12)[0], 14
    if proto in (0x8100, 0x88A8):
        if n < off + 4:
            return 0
        proto = struct.unpack_from(">H", f, off + 2)[0]
        off += 4
        if proto == 0x8100:
            if n < off + 4:
                return 0
            proto = struct.unpack_from(">H", f, off + 2)[0]
            off += 4
    if proto != 0x0800 or n < off + 20:
        return 0
    if not GoldenDataplane._ipv4_header_ok(f, off) or f[off + 9] != 17:
        return 0
    if struct.unpack_from(">H", f, off + 6)[0] & 0x1FFF:
        return 0
    udp = off + (f[off] & 0xF) * 4
    return int(n >= udp + 8 and
               struct.unpack_from(">H", f, udp + 2)[0] == 67)


def run_case(shape, grid_cap, tables, launches, any_order_rows=(), **log2):
    """`launches`: [(frames, now_ns)].  Returns (gpu, cpu) for further
    checks by the case."""
    n, cap, ordered = shape
    gpu, cpu = snap.make_pair(**log2)
    for l in (gpu, cpu):
        tables(l)
    grid_cap(cap)
    for k, (frames, now) in enumerate(launches):
        assert len(frames) == n
        # the shared golden dispatch classifies like the kernel for these
        assert all(snap.is_dhcp(f) == bool(golden_class(f)) for f in frames)
        v, ol, rows = snap.run_uplink(gpu, frames, ordered, now_ns=now)
        want = snap.golden_uplink(cpu, frames, now_ns=now)
        snap.check_rows(frames, want, v, ol, rows,
                        any_order_rows=any_order_rows)
        assert snap.all_stats(gpu) == snap.all_stats(cpu), f"launch {k}"
        assert snap.session_table(gpu) == snap.golden_session_table(cpu)
        assert spoof_events(gpu) == spoof_events(cpu), f"launch {k}"
    return gpu, cpu


def spoof_events(l):
    """Drained ring as a sorted list: ring order is thread order."""
    return sorted((e["timestamp"], bytes(e["src_mac"]), e["protocol"],
                   e["spoofed_ip"], e["allowed_ip"])
                  for e in l.drain_spoof_events())


# ------------------------------------------------------------------- frames
N_SUBS = 40


def tag(f, *tags):
    """Insert VLAN tags (tpid, vid) behind the MAC addresses."""
    return f[:12] + b"".join(struct.pack(">HH", t, v) for t, v in tags) + \
        f[12:]


def l4_frame(k):
    """Subscriber k's one flow: UDP, TCP (checksum at byte 50, outside the
    window), UDP, ICMP; 42-byte frames take the byte parser."""
    return snap.flow_frame(k)


def nat_and_bindings(l, n_subs=N_SUBS, mode=abi.AS_STRICT):
    snap.flow_tables(l, n_subs)
    l.set_antispoof_config(default_mode=abi.AS_DISABLED, log_violations=True)
    for k in range(n_subs):
        l.add_binding(sub_mac(k), ipv4=sub_ip(k), mode=mode)


SHORT_LENS = (13, 14, 33, 34, 47, 48)


def short_frame(i):
    """A 64-byte UDP frame of subscriber i cut to 13, 14, 33, 34, 47 or 48
    bytes: around the Ethernet header, the IPv4 header and the window."""
    k = i % N_SUBS
    f = build_ipv4(sub_mac(k), SERVER_MAC, sub_ip(k), DST, proto=17,
                   sport=21000 + k, dport=53, payload=b"\x00" * 22)
    return f[:SHORT_LENS[i % 6]]


def tagged_frame(i):
    """One flow per subscriber; i and i + N_SUBS tag alike."""
    k = i % N_SUBS
    f = build_ipv4(sub_mac(k), SERVER_MAC, sub_ip(k), DST,
                   proto=(17, 6, 1)[k % 3], sport=22000 + k, dport=53,
                   icmp_id=900 + k, payload=b"\x00" * 22)
    if i % 4 == 3:
        return f                                          # untagged twin
    if i % 2:
        return tag(f, (0x88A8, 200), (0x8100, 30))        # QinQ
    return tag(f, (0x8100, 100))                          # 802.1Q


def l2_frame(i):
    """PPPoE discovery / session and ARP ethertypes, longer and shorter
    than the window; every fourth frame is plain data."""
    k = i % N_SUBS
    if i % 4 == 3:
        return l4_frame(k)
    et = (0x8863, 0x8864, 0x0806)[i % 3]
    body = bytes(range(1, 47)) if i % 2 else bytes(range(1, 29))
    return SERVER_MAC + sub_mac(k) + struct.pack(">H", et) + body


# ==================================================================== cases
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_l4_sessions_created_then_hit(shape, grid_cap):
    """UDP, TCP and ICMP flows behind strict bindings: the first launch
    creates the sessions, the second hits them."""
    n = shape[0]
    frames = [l4_frame(i % N_SUBS) for i in range(n)]
    _, cpu = run_case(shape, grid_cap, nat_and_bindings,
                      [(frames, NOW_NS), (frames, NOW_NS + MS)], sess_log2=6)
    assert cpu.nat_get_stats()["sessions_created"] == min(n, N_SUBS)
    assert cpu.antispoof_get_stats()["packets_allowed"] == 2 * n


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_short_frames(shape, grid_cap):
    n = shape[0]
    frames = [short_frame(i) for i in range(n)]
    if n >= 6:
        assert {len(f) for f in frames} == set(SHORT_LENS)
    run_case(shape, grid_cap, nat_and_bindings, [(frames, NOW_NS)])


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_tagged_frames(shape, grid_cap):
    """802.1Q and QinQ data frames read as non-IP (allowed, not NATed);
    their untagged twins are NATed."""
    n = shape[0]
    frames = [tagged_frame(i) for i in range(n)]
    _, cpu = run_case(shape, grid_cap, nat_and_bindings, [(frames, NOW_NS)])
    if n >= 63:
        st = cpu.nat_get_stats()
        assert 0 < st["packets_snat"] < n


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_pppoe_and_arp_pass(shape, grid_cap):
    n = shape[0]
    frames = [l2_frame(i) for i in range(n)]
    assert {len(f) for f in frames if f[12:14] != b"\x08\x00"} <= {42, 60}
    run_case(shape, grid_cap, nat_and_bindings, [(frames, NOW_NS)])


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_ipv6_with_and_without_v6_binding(shape, grid_cap):
    """snap.binding_frame mixes IPv6 frames of MACs with a bound v6 address
    (right and wrong source) and without one into IPv4 traffic of every
    binding mode."""
    n = shape[0]
    frames = [snap.binding_frame(i) for i in range(n)]
    frames[0] = snap.v6_frame(sub_mac(1), bytes(16))    # loose, no v6 bound
    if n > 2:
        frames[2] = snap.v6_frame(sub_mac(4), bytes(16))  # strict, none bound
    run_case(shape, grid_cap,
             lambda l: snap.binding_tables(l, abi.AS_STRICT),
             [(frames, NOW_NS)], binding_log2=6)


@pytest.mark.parametrize("default_mode", [abi.AS_DISABLED, abi.AS_STRICT,
                                          abi.AS_LOOSE])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_no_binding_under_default_mode(shape, default_mode, grid_cap):
    """Unknown MACs: sources inside and outside the allowed range."""
    n = shape[0]
    frames = [build_ipv4((0xEE1100000000 + i).to_bytes(6, "big"), SERVER_MAC,
                         (ip2u32("10.1.5.5"), SPOOF_SRC)[i % 2], DST,
                         proto=17, sport=4000 + i, dport=53,
                         payload=b"\x00" * (22 if i % 3 else 0))
              for i in range(n)]
    _, cpu = run_case(shape, grid_cap,
                      lambda l: snap.binding_tables(l, default_mode),
                      [(frames, NOW_NS)], binding_log2=6)
    st = cpu.antispoof_get_stats()
    if default_mode == abi.AS_DISABLED:
        assert st["packets_allowed"] == n
    elif n >= 63:
        assert st["packets_dropped"] > 0


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_strict_violation_is_logged_with_the_window_mac(shape, grid_cap):
    """Every other frame spoofs its source; 64-byte frames take the window
    (the logged MAC comes from registers), 42-byte frames the byte parser.
    run_case compares the drained ring with the golden model's events."""
    n = shape[0]
    frames = [build_ipv4(sub_mac(i % N_SUBS), SERVER_MAC,
                         SPOOF_SRC if i % 2 == 0 else sub_ip(i % N_SUBS),
                         DST, proto=17, sport=23000 + i % N_SUBS, dport=53,
                         payload=b"\x00" * (0 if i % 4 == 2 else 22))
              for i in range(n)]
    gpu, cpu = run_case(shape, grid_cap, nat_and_bindings, [(frames, NOW_NS)])
    st = cpu.antispoof_get_stats()
    assert st["packets_logged"] == st["packets_dropped"] == (n + 1) // 2
    # the ring really was compared: drain again after a second, known batch
    one = [frames[0]]
    v, _, _ = snap.run_uplink(gpu, one, False, now_ns=NOW_NS + MS)
    assert v.cpu().tolist() == [DROP]
    assert spoof_events(gpu) == [(NOW_NS + MS, sub_mac(0), 4, SPOOF_SRC,
                                  sub_ip(0))]


# ------------------------------------------------------ subscriber contexts
REFILL = snap.DRY      # the subscriber whose bucket empties, then refills


def ctx_launches(n):
    """Launch 1 (1 ms after the policies were set) empties one bucket: it
    holds three packets and gets more.  Launch 2 comes 150 ms later with
    ONE packet of that subscriber: at 1000 B/s the refill credits 150
    bytes, so the packet passes through the refill path.  (Its other rows
    carry another subscriber's frames in launch 2: how many of several
    racing packets a freshly refilled bucket admits depends on timing.)"""
    first = [snap.ctx_frame(i) for i in range(n)]
    dry = [i for i in range(n) if i % 8 == 3]
    second = list(first)
    for i in dry[1:]:
        second[i] = snap.ctx_frame(8)      # rate-limited, ample bucket
    return dry, [(first, NOW_NS + MS), (second, NOW_NS + 151 * MS)]


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_contexts_and_a_bucket_that_refills(shape, grid_cap):
    """nat_valid and qos_valid each 0 and 1, rate 0, no context
    (snap.ctx_kind), an emptied bucket and its refill."""
    n = shape[0]
    dry, launches = ctx_launches(n)
    gpu, cpu = run_case(shape, grid_cap, snap.ctx_tables, launches,
                        any_order_rows=dry, subnat_log2=6)
    if n >= 63:
        # launch 1: three of the dry rows pass; launch 2: the one passes
        assert cpu.qos_get_stats()["packets_dropped"] == len(dry) - 3
        assert cpu.nat_get_stats()["packets_passed"] > 0


# ------------------------------------------------- probe distance >= 2
def colliding(keys, log2, want):
    """The first `want` keys of `keys` that share one home slot."""
    by = {}
    for k in keys:
        g = by.setdefault(abi.mix64(k) & ((1 << log2) - 1), [])
        g.append(k)
        if len(g) == want:
            return g
    raise AssertionError("no colliding keys")


@functools.lru_cache(maxsize=None)
def far_subscribers():
    """Three (mac, ip) pairs; the MACs share a home slot of a 16-slot
    binding table and the addresses one of a 16-slot context table."""
    macs = colliding((0xAABBCC100000 + j for j in range(4096)), 4, 3)
    ips = colliding((ip2u32("10.1.16.1") + j for j in range(4096)), 4, 3)
    return tuple(zip((m.to_bytes(6, "big") for m in macs), ips))


def far_tables(l):
    l.set_antispoof_config(default_mode=abi.AS_STRICT, log_violations=True)
    for j, (mac, ip) in enumerate(far_subscribers()):
        l.add_binding(mac, ipv4=ip, mode=abi.AS_STRICT)
        l.add_subscriber_nat(ip, ip2u32("203.0.113.7"), 1024 + 512 * j,
                             1535 + 512 * j, subscriber_id=j + 1)
        l.set_qos_policy(ip, 10**9, 1 << 20, direction="ingress",
                         now_ns=NOW_NS)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_keys_at_probe_distance_two(shape, grid_cap):
    """16-slot binding and context tables, three keys on one chain each:
    the third sits two slots from home, so its fields come from a probe
    that is not the first."""
    n = shape[0]
    subs = far_subscribers()
    frames = [build_ipv4(subs[i % 3][0], SERVER_MAC,
                         subs[i % 3][1] if i % 5 else SPOOF_SRC, DST,
                         proto=17, sport=24000, dport=53,
                         payload=b"\x00" * 22) for i in range(n)]
    gpu, _ = run_case(shape, grid_cap, far_tables,
                      [(frames, NOW_NS + MS), (frames, NOW_NS + 2 * MS)],
                      binding_log2=4, subnat_log2=4)
    b = gpu.bindings.cpu().numpy().view("<u8").reshape(16, 4)[:, 0]
    c = gpu.subctx.cpu().numpy().view("<u4").reshape(16, 16)[:, 0]
    for tbl, keys in ((b, [int.from_bytes(m, "big") for m, _ in subs]),
                      (c, [ip for _, ip in subs])):
        dist = [(int(np.nonzero(tbl == k)[0][0]) - (abi.mix64(k) & 15)) % 16
                for k in keys]
        assert max(dist) >= 2, dist


# --------------------------------------------------------------- classifier
def ip_options(f, words=1):
    """Untagged frame with `words` 4-byte NOP options added (IHL 5+words);
    total length adjusted, checksum left alone (nothing here checks it)."""
    tot = struct.unpack_from(">H", f, 16)[0] + 4 * words
    return (f[:14] + bytes([0x45 + words]) + f[15:16] +
            struct.pack(">H", tot) + f[18:34] + b"\x01" * (4 * words) +
            f[34:])


def fragment(f, frag_field):
    return f[:20] + struct.pack(">H", frag_field) + f[22:]


@functools.lru_cache(maxsize=None)
def classifier_frames():
    fr = []
    for i in range(257):
        fr += [l4_frame(i % N_SUBS), short_frame(i), tagged_frame(i),
               l2_frame(i), snap.binding_frame(i), snap.ctx_frame(i),
               snap.dhcp_frame(i)]
    d = build_dhcp_request(sub_mac(1), DHCP_DISCOVER, xid=7)
    r = build_dhcp_request(sub_mac(2), DHCP_REQUEST, xid=8)
    to68 = d[:36] + b"\x00\x44" + d[38:]
    fr += [
        ip_options(d), ip_options(r, 2), ip_options(d, 10),   # IHL 6, 7, 15
        ip_options(to68),
        fragment(d, 0x0010), fragment(d, 0x2010),      # non-first fragments
        fragment(d, 0x2000), fragment(d, 0x4000),      # first fragment, DF
        fragment(ip_options(d), 0x0001),
        build_dhcp_request(sub_mac(3), DHCP_DISCOVER, c_tag=100),
        build_dhcp_request(sub_mac(4), DHCP_REQUEST, s_tag=200, c_tag=30),
        tag(d, (0x88A8, 5)), tag(d, (0x8100, 5), (0x88A8, 6)),
        tag(ip_options(d), (0x8100, 9)),
        d[:41], d[:42], d[:48], ip_options(d)[:45], ip_options(d)[:46],
        tag(d, (0x8100, 5))[:17], tag(d, (0x8100, 5))[:18],
        tag(d, (0x8100, 5))[:45], tag(d, (0x8100, 5))[:46],
        tag(d, (0x88A8, 5), (0x8100, 6))[:21],
        d[:14] + b"\x65" + d[15:], d[:14] + b"\x44" + d[15:],   # v6, ihl 4
        d[:23] + b"\x06" + d[24:],                                  # TCP:67
        d[:12] + b"\x86\xdd" + d[14:],
    ]
    return tuple(fr)


def test_classifier_frames_cover_both_classes():
    fr = classifier_frames()
    cls = [golden_class(f) for f in fr]
    assert 0 < sum(cls) < len(cls)
    tail = cls[-28:]
    assert 0 < sum(tail) < len(tail)
    # IP options, a first fragment and tagged requests are DHCP
    assert golden_class(fr[-28]) == 1 and golden_class(fr[-22]) == 1
    assert golden_class(fr[-19]) == 1 and golden_class(fr[-18]) == 1
    assert golden_class(fr[-24]) == 0           # non-first fragment


@pytest.mark.parametrize("stride", [512, 344, 346])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 0],
                         ids=lambda n: f"n{n}" if n else "all")
def test_pkt_class_equals_golden_class(n, stride):
    """Stride 344 leaves odd rows 8-B but not 16-B aligned, 346 leaves
    them 2-B aligned: the byte-wise walk."""
    import torch
    from bng_amd.dataplane.launcher import HipLauncher
    gpu = HipLauncher(sub_log2=6, sess_log2=6, eim_log2=6, subnat_log2=6,
                      qos_log2=6, binding_log2=6, n_pools=4)
    fr = classifier_frames()
    # the hand-made frames last in the list are in every subset
    frames = fr if n == 0 else fr[-min(n, 28):] + fr[:max(0, n - 28)]
    assert max(len(f) for f in frames) <= stride
    d, l = snap.device_batch(gpu, frames, stride)
    cls = torch.full((len(frames),), 7, dtype=torch.uint8, device=gpu.device)
    gpu.ext.pkt_class(d, l, cls)
    got = cls.cpu().tolist()
    want = [golden_class(f) for f in frames]
    bad = [i for i in range(len(frames)) if got[i] != want[i]]
    assert not bad, [(i, len(frames[i]), frames[i][12:24].hex())
                     for i in bad[:8]]
