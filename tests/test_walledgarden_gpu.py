"""The walled-garden gate on the device: wg_uplink_kernel ahead of the
uplink pipeline, wg_downlink_kernel behind the downlink pipeline, and the
entry CRUD kernels, against GoldenDataplane.garden_uplink / garden_downlink.

Verdicts, gate codes and counters are integers, so every comparison with
the golden model is EXACT, packet by packet.  That needs verdicts that do
not depend on lane order, and the inputs are chosen for it, as in the
accounting suite: QoS buckets are unlimited or the 10-byte, no-refill kind
that always drops, and every NATed subscriber carries one flow.  Equal
DHCP / NAT / antispoof / QoS counters on both sides prove that no gated
frame reached the pipeline.

Subscriber k is quarantined when k % 8 == 0 (no port block, no QoS policy,
like a walled lease), blocked when k % 8 == 4 (WITH a port block: without
the gate it would keep full service), a plain subscriber otherwise.

Shapes: batch sizes around the wave (64) and block (256) edges, and a
forced 2-block grid at n = 2*256*2 + 37 — three grid-stride iterations
with a ragged last wave.  Tables are small (log2 4..13), stride 128.
"""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import DROP, FWD, PASS
from bng_amd.dataplane.packets import (DHCP_DISCOVER, DHCP_REQUEST,
                                       build_dhcp_request, build_ipv4, ip2u32)
from bng_amd.pppoe import codec as C
from wg_frames import (ALLOWED, CORE_MAC, DNS, GATE_NAMES, OTHER, PORTAL,
                       PORTAL_PORT, SERVER_MAC, raw_ipv4)

NOW_SEC = 1_700_000_000
NOW_NS = NOW_SEC * 10**9
NOW2_NS = NOW_NS + 1000
DST = OTHER
STRIDE = 128

FORCED_CAP = 2
FORCED_N = FORCED_CAP * 256 * 2 + 37        # 1061
EDGE_SIZES = [1, 63, 64, 65, 255, 256, 257]
SHAPES = [(n, 0) for n in EDGE_SIZES] + [(FORCED_N, FORCED_CAP)]
ALL_GATES = set(range(6))
WG_DTYPE = np.dtype(abi.WG_ENTRY_DTYPE)


def shape_id(s):
    return f"n{s[0]}-cap{s[1]}"


def sub_mac(k):
    return (0xAABBCC000000 + k).to_bytes(6, "big")


def sub_ip(k):
    return ip2u32("10.1.0.1") + k


def role(k):
    return {0: "walled", 4: "blocked"}.get(k % 8, "plain")


def qos_drops(k):
    return k % 9 == 4           # 10-byte bucket, no refill: always drops


def garden_entries(n, roles=("walled", "blocked")):
    st = {"walled": abi.WG_WALLED, "blocked": abi.WG_BLOCKED}
    return [(sub_ip(k), sub_mac(k), st[role(k)]) for k in range(n)
            if role(k) in roles]


def make_pair(n_subs, roles=("walled", "blocked"), acct=False, wg_log2=13):
    """(HipLauncher, GoldenLauncher) with identical small tables; the
    subscribers whose role is in `roles` are in the garden on both."""
    from bng_amd.dataplane.launcher import GoldenLauncher, HipLauncher
    gpu = HipLauncher(sub_log2=13, sess_log2=13, eim_log2=13, subnat_log2=13,
                      qos_log2=13, binding_log2=13, n_pools=16,
                      pppoe_log2=13, acct_log2=13, wg_log2=wg_log2)
    cpu = GoldenLauncher()
    cpu.dp.now_ns = NOW_NS
    for l in (gpu, cpu):
        l.set_server_config(SERVER_MAC, ip2u32("10.255.255.1"))
        l.add_pool(1, ip2u32("10.1.0.0"), 16, ip2u32("10.1.255.254"),
                   ip2u32("8.8.8.8"), ip2u32("1.1.1.1"), 3600)
        l.set_antispoof_config(default_mode=abi.AS_DISABLED,
                               log_violations=True)
        for k in range(n_subs):
            ip = sub_ip(k)
            l.add_subscriber(sub_mac(k), 1, ip, NOW_SEC + 600)
            l.add_binding(sub_mac(k), ipv4=ip, mode=abi.AS_STRICT)
            if role(k) == "walled":
                continue
            ps = 1024 + (k % 100) * 512
            l.add_subscriber_nat(ip, ip2u32("203.0.113.1") + k // 100,
                                 ps, ps + 511, subscriber_id=k + 1)
            if qos_drops(k):
                l.set_qos_policy(ip, 8000, 10, direction="ingress",
                                 now_ns=NOW_NS)
            else:
                l.set_qos_policy(ip, 0, 0, direction="ingress",
                                 now_ns=NOW_NS)
        l.wg_set_config(ALLOWED)
        l.wg_set(garden_entries(n_subs, roles))          # one launch
        if acct:
            l.acct_add([sub_ip(k) for k in range(n_subs)])
    return gpu, cpu


@pytest.fixture
def grid_cap():
    from bng_amd.dataplane.build import get_ext
    ext = get_ext(required=True)
    try:
        yield ext.set_pkt_grid_cap
    finally:
        ext.set_pkt_grid_cap(0)


# ----------------------------------------------------------------- frames
def f_data(k, length=None):
    """UDP data frame of subscriber k: one flow per subscriber."""
    length = 60 + (k * 7) % 61 if length is None else length
    return build_ipv4(sub_mac(k), SERVER_MAC, sub_ip(k), DST, proto=17,
                      sport=20000 + k, dport=53, payload=bytes(length - 42))


def renewal(k):
    f = build_dhcp_request(sub_mac(k), DHCP_REQUEST, ciaddr=sub_ip(k))
    return f[:26] + sub_ip(k).to_bytes(4, "big") + f[30:]


def wg_up(k, dst, proto, dport=0, mac=None, **kw):
    return raw_ipv4(sub_mac(k) if mac is None else mac, SERVER_MAC,
                    sub_ip(k), dst, proto, 30000 + k, dport, **kw)


WALLED_KINDS = [
    lambda k: wg_up(k, PORTAL, 6, PORTAL_PORT, payload=k % 40),   # ALLOW
    lambda k: wg_up(k, DNS, 17, 53, payload=k % 50),              # ALLOW
    lambda k: wg_up(k, OTHER, 6, 80),                             # REDIRECT
    lambda k: wg_up(k, OTHER, 6, 443, payload=9),                 # DROP_WALLED
    lambda k: wg_up(k, PORTAL, 6, PORTAL_PORT, mac=sub_mac(k + 1)),  # MAC
    lambda k: wg_up(k, PORTAL, 1, payload=16),        # portless ALLOW
    renewal,                                          # NONE: to the pipeline
    lambda k: wg_up(k, PORTAL, 6, PORTAL_PORT, ihl=6),            # ALLOW
    lambda k: wg_up(k, DNS, 17, 53, ihl=8),     # ports straddle two windows
    lambda k: wg_up(k, PORTAL, 6, 443, l4_len=19),    # cut at 53: portless
    lambda k: wg_up(k, OTHER, 17, 53, frag=77),       # fragment elsewhere
    lambda k: wg_up(k, OTHER, 6, 8080, ihl=12),       # l4 at 62: REDIRECT
    lambda k: wg_up(k, DNS, 6, 53, ihl=15, payload=3),    # l4 at 74
    lambda k: wg_up(k, OTHER, 6, 80, ihl=6, l4_len=19),   # cut: DROP_WALLED
]


def mix_frame(i):
    """Packet i comes from subscriber i."""
    if role(i) == "walled":
        return WALLED_KINDS[(i // 8) % len(WALLED_KINDS)](i)
    if role(i) == "blocked":
        return f_data(i)                     # would SNAT and forward
    if i % 10 == 9:
        return build_dhcp_request(sub_mac(i), DHCP_DISCOVER, xid=0x1000 + i)
    if i % 32 == 3:
        return SERVER_MAC + sub_mac(i) + b"\x08\x06" + bytes(28)     # ARP
    if i % 32 == 6:                          # VLAN-tagged data frame
        f = f_data(i)
        return f[:12] + b"\x81\x00\x00\x64" + f[12:]
    return f_data(i)


def is_dhcp(f):
    return (len(f) >= 42 and f[12:14] == b"\x08\x00" and f[14] == 0x45 and
            f[23] == 17 and f[36:38] == b"\x00\x43")


# ----------------------------------------------------------- golden chain
def golden_uplink(cpu, frames, now_ns=NOW_NS, stride=STRIDE):
    """HipLauncher.uplink's sequence on the golden model: decap, resolve,
    the gate, the fused kernel's dispatch for what the gate left alone,
    REJECT -> DROP, commit.  Returns (verdicts, gates, out_lens, frames as
    the gate saw them)."""
    dp = cpu.dp
    verdicts, gates, out_lens, seen = [], [], [], []
    for f in frames:
        dp.now_ns = now_ns
        f = f[:stride]
        fb = bytearray(f)
        st, L = dp.pppoe_decap(fb) if dp.pppoe_sessions \
            else (abi.PPPOE_NONE, len(f))
        g = bytes(fb[:L]) if st == abi.PPPOE_DECAP else f
        key = dp.acct_resolve(g, "src")
        out_len = len(g)
        gate, v = dp.garden_uplink(g) if dp.wg else (abi.WG_NONE, None)
        et = struct.unpack_from(">H", g, 12)[0] if len(g) >= 14 else 0
        if gate != abi.WG_NONE:
            pass
        elif et in (0x8863, 0x8864, 0x0806):
            v = PASS
        elif is_dhcp(g):
            v, out_len = dp.dhcp_fastpath(bytearray(g))
        else:
            fb = bytearray(g)
            v = dp.antispoof(bytes(fb))
            if v == FWD:
                v = dp.nat44_egress(fb)
            if v == FWD:
                v = dp.qos(g, "ingress")
        if st == abi.PPPOE_REJECT:
            v = DROP
        dp.acct_commit(key, "uplink", out_len, v, now_ns)
        verdicts.append(v)
        gates.append(gate)
        out_lens.append(out_len)
        seen.append(g)
    return verdicts, gates, out_lens, seen


def golden_downlink(cpu, frames, now_ns=NOW2_NS):
    dp = cpu.dp
    verdicts, gates = [], []
    for f in frames:
        dp.now_ns = now_ns
        fb = bytearray(f)
        v = dp.nat44_ingress(fb)
        if v == FWD:
            v = dp.qos(bytes(fb), "egress")
        gate, v = dp.garden_downlink(fb, v) if dp.wg else (abi.WG_NONE, v)
        dp.acct_commit(dp.acct_resolve(fb, "dst"), "downlink", len(fb), v,
                       now_ns)
        if dp.pppoe_sessions:
            _st, v, _L = dp.pppoe_encap(fb, v, STRIDE)
        verdicts.append(v)
        gates.append(gate)
    return verdicts, gates


def all_stats(l):
    return {"dhcp": l.get_stats(), "nat": l.nat_get_stats(),
            "qos": l.qos_get_stats(), "antispoof": l.antispoof_get_stats(),
            "walledgarden": l.wg_get_stats()}


def names(gates):
    return [GATE_NAMES[g] for g in gates]


def run_uplink(gpu, cpu, frames, what, **kw):
    """One batch through both; asserts verdicts, gates, out_len, the rows
    of every gated frame and every counter agree.  Returns (verdicts,
    gates, the batch's rows after the pipeline)."""
    data, lens = gpu.make_batch(list(frames), stride=STRIDE)
    v, ol = gpu.uplink(data, lens, now_ns=NOW_NS, now_sec=NOW_SEC, **kw)
    vc, gc, oc, seen = golden_uplink(cpu, frames)
    got_g = gpu.last_wg_gate.cpu().tolist()
    assert names(got_g) == names(gc), f"{what}: gates differ"
    assert v.cpu().tolist() == vc, f"{what}: verdicts differ"
    assert ol.cpu().numpy().view(np.uint16).tolist() == oc, \
        f"{what}: out_len differs"
    host = data.cpu().numpy()
    for i, (g, f) in enumerate(zip(gc, seen)):
        if g != abi.WG_NONE:
            assert oc[i] == len(f)
            assert host[i, :len(f)].tobytes() == f, \
                f"{what}: packet {i} ({GATE_NAMES[g]}) was rewritten"
    got, want = all_stats(gpu), all_stats(cpu)
    assert got == want, f"{what}: counters differ"
    return vc, gc, host


# ------------------------------------------------------ uplink differential
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_uplink_matches_golden(shape, grid_cap):
    n, cap = shape
    frames = [mix_frame(i) for i in range(n)]
    gpu, cpu = make_pair(n)
    grid_cap(cap)
    for launch in (1, 2):
        # the second batch catches a stale order_out or a stale gate
        vc, gc, _ = run_uplink(gpu, cpu, frames, f"launch {launch}")
        print(f"launch {launch}: {gpu.wg_get_stats()}")
    assert gpu.wg_launches == {"uplink": 2, "downlink": 0}
    assert gpu.wg_count == cpu.wg_count == len(gpu.wg_export())
    if n >= 63:
        assert set(gc) == ALL_GATES          # an all-NONE gate cannot pass
        assert {PASS, FWD, DROP} <= set(vc)
        st = cpu.wg_get_stats()
        assert all(st[k] > 0 for k in abi.WG_STAT_NAMES[:5])
        assert all(st[k] == 0 for k in abi.WG_STAT_NAMES[5:])
        # no session for a blocked subscriber, port block or not
        blocked = {sub_ip(k) for k in range(n) if role(k) == "blocked"}
        assert blocked and not any(key[0] in blocked
                                   for key in cpu.dp.nat_sessions)
        assert cpu.nat_get_stats()["sessions_created"] > 0
        # a quarantined renewal still reaches the pipeline
        assert any(g == abi.WG_NONE and role(i) == "walled"
                   for i, g in enumerate(gc))


def test_dhcp_reply_at_full_stride():
    """Stride 128 cuts every DHCP frame short; at 512 the renewal of a
    quarantined subscriber is answered on the device (gate NONE, TX)."""
    n = 65
    frames = [mix_frame(i) for i in range(n)]
    gpu, cpu = make_pair(n)
    data, lens = gpu.make_batch(list(frames), stride=512)
    v, ol = gpu.uplink(data, lens, now_ns=NOW_NS, now_sec=NOW_SEC)
    vc, gc, oc, _ = golden_uplink(cpu, frames, stride=512)
    assert v.cpu().tolist() == vc
    assert gpu.last_wg_gate.cpu().tolist() == gc
    k = 8 * 6                                # the renewal's subscriber
    assert frames[k] == renewal(k) and gc[k] == abi.WG_NONE
    assert vc[k] == abi.TX
    assert all_stats(gpu) == all_stats(cpu)


# -------------------------------------------------------- order composition
@pytest.mark.parametrize("n", [65, 257])
def test_order_composition(n):
    import torch
    frames = [mix_frame(i) for i in range(n)]
    rng = np.random.default_rng(11)
    seen = []
    for mode in ("plain", "sort", "shuffled"):
        gpu, cpu = make_pair(n)
        kw = {}
        if mode == "sort":
            kw["sort_by_type"] = True
        elif mode == "shuffled":
            kw["order"] = torch.from_numpy(
                rng.permutation(n).astype(np.int32)).to(gpu.device)
        vc, gc, _ = run_uplink(gpu, cpu, frames, mode, **kw)
        seen.append((vc, gc))
    assert seen[0] == seen[1] == seen[2]
    assert set(seen[0][1]) == ALL_GATES


def test_out_of_range_order_entries_pass_through():
    """A caller's order may hold entries outside [0, n): the gate hands
    them on unchanged and the pipeline skips them, as it always did."""
    import torch
    n = 70
    frames = [mix_frame(i) for i in range(n)]
    gpu, cpu = make_pair(n)
    order = np.arange(n, dtype=np.int32)
    skipped = [1, 2, 9, 64]                  # a walled one among them
    order[skipped] = [-1, n, -7, 2**31 - 1]
    data, lens = gpu.make_batch(list(frames), stride=STRIDE)
    v, _ = gpu.uplink(data, lens, now_ns=NOW_NS, now_sec=NOW_SEC,
                      order=torch.from_numpy(order).to(gpu.device))
    keep = [i for i in range(n) if i not in skipped]
    vc, gc, _, _ = golden_uplink(cpu, [frames[i] for i in keep])
    got_v, got_g = v.cpu().tolist(), gpu.last_wg_gate.cpu().tolist()
    assert [got_v[i] for i in keep] == vc
    assert [got_g[i] for i in keep] == gc
    assert [got_v[i] for i in skipped] == [0] * 4
    assert [got_g[i] for i in skipped] == [abi.WG_NONE] * 4
    assert all_stats(gpu) == all_stats(cpu)


# ----------------------------------------------------------------- downlink
def return_frame(row, length):
    """The core's answer to a forwarded (SNAT-ed) UDP frame."""
    nat_ip = struct.unpack_from(">I", row, 26)[0]
    nat_port = struct.unpack_from(">H", row, 34)[0]
    return build_ipv4(CORE_MAC, SERVER_MAC, DST, nat_ip, proto=17, sport=53,
                      dport=nat_port, payload=bytes(length - 42))


def wg_down(k, src, proto, sport=0, **kw):
    return raw_ipv4(CORE_MAC, SERVER_MAC, src, sub_ip(k), proto, sport,
                    30000 + k, **kw)


DOWN_KINDS = [
    lambda k: wg_down(k, DNS, 17, 53, payload=20),            # ALLOW
    lambda k: wg_down(k, OTHER, 6, 80, payload=5),            # DROP_WALLED
    lambda k: wg_down(k, PORTAL, 1, payload=8),               # ALLOW
    lambda k: wg_down(k, OTHER, 17, 53, frag=9),              # DROP_WALLED
    lambda k: wg_down(k, PORTAL, 6, PORTAL_PORT, ihl=8),      # ALLOW
    lambda k: wg_down(k, PORTAL, 6, 443),                     # DROP_WALLED
]


@pytest.mark.parametrize("shape", [(65, 0), (256 + 37, 1)], ids=shape_id)
def test_downlink_matches_golden(shape, grid_cap):
    n, cap = shape
    # the blocked subscribers join the garden only after their sessions
    # exist: the gate must stop return traffic through a LIVE session
    gpu, cpu = make_pair(n, roles=("walled",))
    natted = [k for k in range(n) if role(k) != "walled"]
    up = [f_data(k) for k in natted]
    vu, _, host = run_uplink(gpu, cpu, up, "uplink")
    assert set(vu) == {FWD, DROP}            # QoS drops behind SNAT
    for l in (gpu, cpu):
        l.wg_set(garden_entries(n, roles=("blocked",)))
    back = []
    for k in range(n):
        if role(k) == "walled":
            back.append(DOWN_KINDS[(k // 8) % len(DOWN_KINDS)](k))
        else:
            back.append(return_frame(host[natted.index(k)],
                                     60 + (k * 5) % 60))
    stray = build_ipv4(CORE_MAC, SERVER_MAC, DST, ip2u32("203.0.113.1"),
                       proto=17, sport=53, dport=60001, payload=bytes(30))
    back.insert(len(back) // 2, stray)       # to nobody in the garden
    grid_cap(cap)
    for launch in (1, 2):
        d2, l2 = gpu.make_batch(back, stride=STRIDE)
        v = gpu.downlink(d2, l2, now_ns=NOW2_NS)
        vc, gc = golden_downlink(cpu, back)
        assert names(gpu.last_wg_gate.cpu().tolist()) == names(gc), \
            f"launch {launch}: gates differ"
        assert v.cpu().tolist() == vc, f"launch {launch}: verdicts differ"
        assert all_stats(gpu) == all_stats(cpu)
    assert set(gc) == {abi.WG_NONE, abi.WG_ALLOW, abi.WG_DROP_WALLED,
                       abi.WG_DROP_BLOCKED}
    assert {FWD, DROP} <= set(vc)
    st = cpu.wg_get_stats()
    assert all(st[k] > 0 for k in abi.WG_STAT_NAMES[5:])
    assert cpu.nat_get_stats()["packets_dnat"] > 0
    assert gpu.wg_launches["downlink"] == 2


# ---------------------------------------------------------- with accounting
def test_quarantined_subscribers_are_accounted():
    n = 257
    frames = [mix_frame(i) for i in range(n)]
    gpu, cpu = make_pair(n, acct=True)
    run_uplink(gpu, cpu, frames, "uplink")
    ips = [sub_ip(k) for k in range(n)]
    got, want = gpu.acct_read(ips), cpu.acct_read(ips)
    for k, (g, w) in enumerate(zip(got, want)):
        assert tuple(int(x) for x in g) == tuple(int(x) for x in w), \
            f"entry of subscriber {k} ({role(k)})"
    walled = np.array([role(k) == "walled" for k in range(n)])
    blocked = np.array([role(k) == "blocked" for k in range(n)])
    assert (want["up_pkts"][walled] > 0).any()          # ALLOW is billed
    assert (want["up_drop_pkts"][walled] > 0).any()     # drops are counted
    assert (want["up_drop_pkts"][blocked] == 1).all()
    assert (want["up_pkts"][blocked] == 0).all()
    assert gpu.acct_launches == {"resolve": 1, "commit": 1, "downlink": 0}


# -------------------------------------------------------------------- PPPoE
def wrap(frame, sid):
    return C.SessionPacket(sid, C.PROTO_IPV4, frame[14:], src_mac=frame[6:12],
                           dst_mac=frame[0:6]).encode()


def test_quarantined_pppoe_session():
    sid, k = 0x0021, 0
    assert role(k) == "walled"
    gpu, cpu = make_pair(3)
    for l in (gpu, cpu):
        l.add_pppoe_session(sid, sub_mac(k), sub_ip(k))
    portal = wg_up(k, PORTAL, 6, PORTAL_PORT, payload=11)
    up = [wrap(portal, sid), wrap(wg_up(k, OTHER, 6, 443), sid),
          wrap(wg_up(k, OTHER, 6, 80), sid), f_data(1)]
    vc, gc, host = run_uplink(gpu, cpu, up, "uplink")
    assert vc == [FWD, DROP, PASS, FWD]
    assert gc == [abi.WG_ALLOW, abi.WG_DROP_WALLED, abi.WG_REDIRECT,
                  abi.WG_NONE]
    assert gpu.last_pppoe_state.cpu().tolist() == [abi.PPPOE_DECAP] * 3 + \
        [abi.PPPOE_NONE]
    assert host[0, :len(portal)].tobytes() == portal    # decapsulated, no NAT

    back = [wg_down(k, PORTAL, 6, PORTAL_PORT, payload=13),
            wg_down(k, OTHER, 6, 443)]
    d2, l2 = gpu.make_batch(back, stride=STRIDE)
    v = gpu.downlink(d2, l2, now_ns=NOW2_NS)
    vcd, gcd = golden_downlink(cpu, back)
    assert v.cpu().tolist() == vcd == [FWD, DROP]
    assert gpu.last_wg_gate.cpu().tolist() == gcd == [
        abi.WG_ALLOW, abi.WG_DROP_WALLED]
    assert gpu.last_pppoe_state.cpu().tolist() == [abi.PPPOE_ENCAP,
                                                   abi.PPPOE_NONE]
    assert l2.cpu().numpy().view(np.uint16).tolist() == [len(back[0]) + 8,
                                                         len(back[1])]
    assert all_stats(gpu) == all_stats(cpu)
    assert gpu.pppoe_get_stats() == cpu.pppoe_get_stats()


# --------------------------------------------------------------- off is off
class PipelineSpy:
    """Stands in for the extension; records the `order` each pipeline
    launch received."""

    def __init__(self, ext):
        self._ext = ext
        self.orders = []

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def uplink_pipeline(self, *a, **kw):
        self.orders.append(kw.get("order"))
        return self._ext.uplink_pipeline(*a, **kw)


def test_off_means_off():
    import torch
    n = 70
    never, _ = make_pair(n, roles=())
    was, _ = make_pair(n, roles=())
    for l in (never, was):
        l.ext = PipelineSpy(l.ext)
    assert never.wg is None and never.wg_count == 0
    assert len(never.wg_export()) == 0
    up = [mix_frame(i) for i in range(n)]
    down = [wg_down(0, OTHER, 6, 80), wg_down(0, DNS, 17, 53),
            wg_down(4, DNS, 17, 53)]
    order = torch.from_numpy(
        np.random.default_rng(3).permutation(n).astype(np.int32)
    ).to(was.device)

    def both_ways(l):
        d, ln = l.make_batch(up, stride=STRIDE)
        v, ol = l.uplink(d, ln, now_ns=NOW_NS, now_sec=NOW_SEC, order=order)
        d2, l2 = l.make_batch(down, stride=STRIDE)
        v2 = l.downlink(d2, l2, now_ns=NOW2_NS)
        return [t.cpu().numpy() for t in (v, ol, d, ln, v2, d2, l2)]

    # empty garden: the caller's order object reaches the pipeline
    both_ways(was)
    assert was.ext.orders[0] is order and was.ext.orders[1] is None
    assert was.wg_launches == {"uplink": 0, "downlink": 0}
    assert was.last_wg_gate is None

    was.wg_set(garden_entries(n))
    assert was.wg_count == len(garden_entries(n)) > 0
    both_ways(was)
    assert was.ext.orders[2] is not order
    assert was.wg_launches == {"uplink": 1, "downlink": 1}
    assert was.wg_get_stats()["up_drop_blocked"] > 0

    was.wg_remove([e[0] for e in garden_entries(n)])
    assert was.wg_count == 0 and len(was.wg_export()) == 0
    # same NAT state on both from here on: `never` catches up first
    both_ways(never)
    both_ways(never)
    a, b = both_ways(never), both_ways(was)
    assert was.ext.orders[-2] is order
    assert was.wg_launches == {"uplink": 1, "downlink": 1}
    assert never.wg is None
    assert never.wg_launches == {"uplink": 0, "downlink": 0}
    # v, out_len and lens agree; the rows differ only in NAT ports chosen
    # while `was` had its blocked subscribers gated, so compare verdicts
    for x, y in zip((a[0], a[3], a[4], a[6]), (b[0], b[3], b[4], b[6])):
        assert (x == y).all()


# --------------------------------------------------------------------- CRUD
def colliding_ips(log2, count):
    """`count` addresses whose garden keys share one home slot."""
    mask = (1 << log2) - 1
    by_slot = {}
    ip = ip2u32("10.7.0.1")
    while True:
        s = by_slot.setdefault(abi.mix64(abi.wg_key(ip)) & mask, [])
        s.append(ip)
        if len(s) == count:
            return s
        ip += 1


def gate_of(gpu, frames):
    data, lens = gpu.make_batch(frames, stride=STRIDE)
    gpu.uplink(data, lens, now_ns=NOW_NS, now_sec=NOW_SEC)
    return gpu.last_wg_gate.cpu().tolist()


def test_table_lifecycle():
    from bng_amd.dataplane.launcher import GoldenLauncher, HipLauncher
    gpu = HipLauncher(sub_log2=13, sess_log2=13, eim_log2=13, subnat_log2=13,
                      qos_log2=13, binding_log2=13, n_pools=16,
                      pppoe_log2=13, acct_log2=13, wg_log2=4)
    cpu = GoldenLauncher(wg_log2=4)
    a, b, c = colliding_ips(4, 3)
    mac = bytes.fromhex("aabbcc000001")

    def probe(ip):
        return raw_ipv4(mac, SERVER_MAC, ip, PORTAL, 6, 1234, PORTAL_PORT)

    for l in (gpu, cpu):
        l.wg_set_config(ALLOWED)
        l.wg_set([(a, mac, abi.WG_WALLED), (b, mac, abi.WG_WALLED),
                  (c, mac, abi.WG_BLOCKED)])
        assert l.wg_count == 3 == len(l.wg_export())
    assert gate_of(gpu, [probe(a), probe(b), probe(c)]) == [
        abi.WG_ALLOW, abi.WG_ALLOW, abi.WG_DROP_BLOCKED]

    for l in (gpu, cpu):
        l.wg_set([(b, mac, abi.WG_BLOCKED)])             # in place
        assert l.wg_count == 3 == len(l.wg_export())
        row = l.wg_export()
        row = row[row["key"] == abi.wg_key(b)]
        assert [int(x) for x in row["mac_state"]] == [
            abi.wg_mac_state(abi.mac_to_u64(mac), abi.WG_BLOCKED)]
        l.wg_remove([a])
        assert l.wg_count == 2 == len(l.wg_export())
    # b and c are found behind a's tombstone
    assert gate_of(gpu, [probe(a), probe(b), probe(c)]) == [
        abi.WG_NONE, abi.WG_DROP_BLOCKED, abi.WG_DROP_BLOCKED]
    blob = gpu.wg.cpu().numpy().view(WG_DTYPE)
    assert (blob["key"] == abi.KEY_TOMBSTONE).sum() == 1

    for l in (gpu, cpu):
        l.wg_set([(a, mac, abi.WG_WALLED)])              # reuses the tombstone
        assert l.wg_count == 3 == len(l.wg_export())
    blob = gpu.wg.cpu().numpy().view(WG_DTYPE)
    assert (blob["key"] == abi.KEY_TOMBSTONE).sum() == 0
    assert sorted(int(k) for k in gpu.wg_export()["key"]) == sorted(
        int(k) for k in cpu.wg_export()["key"])
    assert gate_of(gpu, [probe(a)]) == [abi.WG_ALLOW]

    # 16 slots: the 17th distinct address finds none within the probe bound
    more = [(ip2u32("10.8.0.1") + i, mac, abi.WG_WALLED) for i in range(13)]
    gpu.wg_set(more)
    assert gpu.wg_count == 16 == len(gpu.wg_export())
    with pytest.raises(RuntimeError, match="wg_log2"):
        gpu.wg_set([(ip2u32("10.9.0.1"), mac, abi.WG_WALLED)])
    assert gpu.wg_count == 16 == len(gpu.wg_export())
    with pytest.raises(ValueError, match="repeat"):
        gpu.wg_set([(a, mac, abi.WG_WALLED), (a, mac, abi.WG_BLOCKED)])


def test_config_limits_and_device_search():
    """A full allow-list on the device: first and last key hit, keys that
    differ in one field only miss."""
    from bng_amd.dataplane.launcher import HipLauncher
    gpu = HipLauncher(sub_log2=13, sess_log2=13, eim_log2=13, subnat_log2=13,
                      qos_log2=13, binding_log2=13, n_pools=16,
                      pppoe_log2=13, acct_log2=13, wg_log2=8)
    keys = [(ip2u32("10.9.0.0") + 7 * i, 1000 + i, 6 if i % 2 else 17)
            for i in range(64)]
    mac = bytes.fromhex("aabbcc000001")
    src = ip2u32("10.1.0.1")
    gpu.wg_set([(src, mac, abi.WG_WALLED)])

    def probe(ip, port, proto, **kw):
        return raw_ipv4(mac, SERVER_MAC, src, ip, proto, 1234, port, **kw)

    with pytest.raises(ValueError):
        gpu.wg_set_config(keys + [(1, 1, 6)])
    with pytest.raises(ValueError):
        gpu.wg_set_config(keys, redirect_ports=range(1, 10))
    for n_keys in (0, 1, 64):
        gpu.wg_set_config(keys[:n_keys] + keys[:n_keys // 2],   # folds
                          redirect_ports=(8000,))
        frames, want = [], []
        for i in ([0, n_keys - 1] if n_keys else []):
            ip, port, proto = keys[i]
            frames += [probe(ip, port, proto), probe(ip, port + 1, proto),
                       probe(ip, port, 23 - proto), probe(ip, 0, 1),
                       probe(ip + 1, port, proto)]
            want += [abi.WG_ALLOW, abi.WG_DROP_WALLED, abi.WG_DROP_WALLED,
                     abi.WG_ALLOW, abi.WG_DROP_WALLED]
        frames += [probe(OTHER, 8000, 6), probe(OTHER, 80, 6),
                   probe(OTHER, 0, 1)]
        want += [abi.WG_REDIRECT, abi.WG_DROP_WALLED, abi.WG_DROP_WALLED]
        assert names(gate_of(gpu, frames)) == names(want), n_keys
