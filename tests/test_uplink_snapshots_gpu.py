"""Fused uplink kernel against the golden model, byte for byte.

The kernel builds DHCP replies in registers and stores them 16 B at a time
when the fast parse ran (untagged frame, 16-B aligned row), byte-wise
otherwise; how it fetches session, binding and subscriber-context entries
is the other thing that gets tuned.  None of that may change a verdict, a
packet byte, a counter or a table entry, so every case here goes through
`launcher.uplink`, with and without an `order` array, at n = 1, 63, 64,
65 and 257, and is compared with `GoldenDataplane`:

  * verdict and out_len of every packet,
  * every byte of every row up to max(len, out_len),
  * every byte past that up to the stride: rows are pre-filled with a
    sentinel, and a builder that stores wider than it should shows there,
  * the four counter groups, exactly.

Tables have 64 slots where the case is about probe chains, so hits land
both on and past the first slot of a chain.  Every batch carries at most
one flow per subscriber, which makes NAT port allocation deterministic.
"""
import functools
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import FWD, PASS, TX
from bng_amd.dataplane.packets import (DHCP_DISCOVER, DHCP_REQUEST,
                                       build_dhcp_request, build_ipv4, ip2u32)

NOW_SEC = 1_700_000_000
NOW_NS = NOW_SEC * 10**9
MS = 10**6
SERVER_MAC = bytes.fromhex("020000000001")
SERVER_IP = ip2u32("10.255.255.1")
DST = ip2u32("93.184.216.34")
PUBLIC_SRC = ip2u32("8.8.4.4")       # not private: NAT forwards untouched
SPOOF_SRC = ip2u32("66.6.6.6")
SENTINEL = 0xA5

SIZES = [1, 63, 64, 65, 257]
SHAPES = [(n, o) for n in SIZES for o in (False, True)]


def shape_id(s):
    return f"n{s[0]}-{'order' if s[1] else 'plain'}"


def sub_mac(k):
    return (0xAABBCC000000 + k).to_bytes(6, "big")


def sub_ip(k):
    return ip2u32("10.1.0.1") + k


# ---------------------------------------------------------------- plumbing
def configure(l):
    """Server and pools; pools 1, 2, 3 have two, one and no DNS server:
    three reply lengths."""
    l.set_server_config(SERVER_MAC, SERVER_IP)
    l.add_pool(1, ip2u32("10.1.0.0"), 16, ip2u32("10.1.255.254"),
               ip2u32("8.8.8.8"), ip2u32("1.1.1.1"), 3600)
    l.add_pool(2, ip2u32("10.1.0.0"), 16, ip2u32("10.1.255.254"),
               ip2u32("9.9.9.9"), 0, 7200)
    l.add_pool(3, ip2u32("10.1.0.0"), 20, ip2u32("10.1.255.254"),
               0, 0, 86400)
    l.set_antispoof_config(default_mode=abi.AS_DISABLED, log_violations=True)
    return l


def golden_launcher():
    from bng_amd.dataplane.launcher import GoldenLauncher
    cpu = GoldenLauncher()
    cpu.dp.now_ns = NOW_NS
    return configure(cpu)


def hip_launcher(**log2):
    from bng_amd.dataplane.launcher import HipLauncher
    sizes = dict(sub_log2=10, sess_log2=10, eim_log2=10, subnat_log2=10,
                 qos_log2=6, binding_log2=10, n_pools=16)
    sizes.update(log2)
    return configure(HipLauncher(**sizes))


def make_pair(**log2):
    return hip_launcher(**log2), golden_launcher()


def is_dhcp(f):
    """The kernel's classification, tags included."""
    if len(f) < 14:
        return False
    off, et = 14, struct.unpack_from(">H", f, 12)[0]
    if et in (0x8100, 0x88A8):
        if len(f) < 18:
            return False
        et2 = struct.unpack_from(">H", f, 16)[0]
        off = 18
        if et2 == 0x8100:
            if len(f) < 22:
                return False
            et2 = struct.unpack_from(">H", f, 20)[0]
            off = 22
        et = et2
    if et != 0x0800 or len(f) < off + 20 or f[off + 9] != 17:
        return False
    l4 = off + (f[off] & 0xF) * 4
    return len(f) >= l4 + 8 and f[l4 + 2:l4 + 4] == b"\x00\x43"


def golden_uplink(cpu, frames, now_ns=NOW_NS):
    """The fused kernel's dispatch on the golden model:
    [(verdict, out_len, bytes)] per frame."""
    out = []
    for f in frames:
        cpu.dp.now_ns = now_ns
        fb = bytearray(f)
        et = struct.unpack_from(">H", f, 12)[0] if len(f) >= 14 else 0
        if et in (0x8863, 0x8864, 0x0806):
            out.append((PASS, len(f), bytes(fb)))
        elif is_dhcp(f):
            v, L = cpu.dp.dhcp_fastpath(fb)
            out.append((v, L, bytes(fb)))
        else:
            v = cpu.dp.antispoof(bytes(fb))
            tagged = et in (0x8100, 0x88A8)
            if v == FWD and not tagged:
                v = cpu.dp.nat44_egress(fb)
                if v == FWD:
                    # keyed by the subscriber's own address: the kernel
                    # reuses the context it probed before the SNAT rewrite
                    v = cpu.dp.qos(bytes(f), "ingress")
            out.append((v, len(f), bytes(fb)))
    return out


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


def type_order(gpu, frames):
    import torch
    cls = np.array([1 if is_dhcp(f) else 0 for f in frames])
    return torch.from_numpy(
        np.argsort(cls, kind="stable").astype(np.int32)).to(gpu.device)


def check_rows(frames, want, v, ol, rows, any_order_rows=()):
    """verdicts, out_len, bytes and untouched sentinel of every row.
    any_order_rows: rows whose verdicts are compared as a multiset."""
    stride = rows.shape[1]
    v, ol = v.cpu().tolist(), (ol.cpu().numpy().view(np.uint16)).tolist()
    free = set(any_order_rows)
    for i, (f, (wv, wl, wb)) in enumerate(zip(frames, want)):
        if i not in free:
            assert v[i] == wv, f"row {i}: verdict {v[i]} != {wv}"
        assert ol[i] == min(wl, stride), f"row {i}: out_len {ol[i]} != {wl}"
        m = max(len(f), ol[i])
        got = rows[i, :m].tobytes()
        if got != wb[:m]:
            bad = [j for j in range(m) if got[j] != wb[j]]
            raise AssertionError(
                f"row {i}: bytes differ at {bad[:16]} (len {len(f)}, "
                f"out_len {ol[i]})")
        past = rows[i, m:]
        assert (past == SENTINEL).all(), (
            f"row {i}: bytes past {m} written at "
            f"{(np.nonzero(past != SENTINEL)[0][:8] + m).tolist()}")
    assert sorted(v[i] for i in free) == sorted(want[i][0] for i in free)


def all_stats(l):
    return {"dhcp": l.get_stats(), "nat": l.nat_get_stats(),
            "qos": l.qos_get_stats(), "antispoof": l.antispoof_get_stats()}


def run_uplink(gpu, frames, ordered, now_ns=NOW_NS, stride=512):
    d, l = device_batch(gpu, frames, stride)
    order = type_order(gpu, frames) if ordered else None
    v, ol = gpu.uplink(d, l, now_ns=now_ns, now_sec=NOW_SEC, order=order)
    return v, ol, d.cpu().numpy()


# ==================================================================== DHCP
N_DHCP_SUBS = 48
CIRCUIT = b"olt-7/1/3:%02d"


def dhcp_tables(l):
    for k in range(N_DHCP_SUBS):
        l.add_subscriber(sub_mac(k), 1 + k % 3, sub_ip(k), NOW_SEC + 600)
    l.add_circuit_subscriber(CIRCUIT % 1, 2, ip2u32("10.1.9.1"),
                             NOW_SEC + 600)
    l.add_vlan_subscriber(100, 0, 3, ip2u32("10.1.9.2"), NOW_SEC + 600)
    l.add_vlan_subscriber(200, 30, 1, ip2u32("10.1.9.3"), NOW_SEC + 600)


def dhcp_frame(k):
    """Request shapes, cycled by k; the subscriber (and with it the pool:
    two, one or no DNS server) cycles independently."""
    mac = sub_mac(k % N_DHCP_SUBS)
    mt = DHCP_DISCOVER if k % 2 else DHCP_REQUEST
    shape = k % 16
    kw = {}
    if shape == 1:
        kw = dict(broadcast=True)
    elif shape == 2:
        kw = dict(ciaddr=sub_ip(k % N_DHCP_SUBS))            # unicast
    elif shape == 3:
        kw = dict(ciaddr=sub_ip(k % N_DHCP_SUBS), broadcast=True)
    elif shape == 4:
        kw = dict(giaddr=ip2u32("10.9.0.1"), src_mac=bytes.fromhex(
            "0299aabbcc01"))                                 # relayed
    elif shape == 5:
        kw = dict(circuit_id=CIRCUIT % 1)                    # known circuit
    elif shape == 6:
        kw = dict(circuit_id=CIRCUIT % 2)                    # falls to MAC
    elif shape in (7, 8, 9):
        kw = dict(pad_before_53=shape - 6)
    elif shape == 10:
        # request longer than any reply: old bytes past the reply stay
        kw = dict(extra_opts=bytes([12, 40]) + b"h" * 40 +
                  bytes([55, 8]) + bytes(range(1, 9)))
    elif shape == 11:
        kw = dict(c_tag=100)                                 # 802.1Q
    elif shape == 12:
        kw = dict(s_tag=200, c_tag=30)                       # QinQ
    elif shape == 13:
        kw = dict(s_tag=300, c_tag=31)             # unknown tags: by MAC
    elif shape == 14:
        mac = (0xEE0000000000 + k).to_bytes(6, "big")        # miss
    elif shape == 15:
        kw = dict(giaddr=ip2u32("10.9.0.2"), pad_before_53=2,
                  circuit_id=CIRCUIT % 1, broadcast=True)
    return build_dhcp_request(mac, mt, xid=0x5000 + k, **kw)


def filler(k):
    """Stateless data frame (public source: forwarded untouched), so an
    `order` array has two classes to sort."""
    return build_ipv4(sub_mac(k % N_DHCP_SUBS), SERVER_MAC, PUBLIC_SRC, DST,
                      proto=17, sport=30000 + k, dport=53,
                      payload=b"\x00" * 22)


@functools.lru_cache(maxsize=None)
def dhcp_frames(n, with_filler=True):
    return tuple(filler(k) if with_filler and k % 5 == 4 else dhcp_frame(k)
                 for k in range(n))


@functools.lru_cache(maxsize=None)
def dhcp_reference(n, with_filler=True):
    """(rows, dhcp stats of ONE pass) from the golden model, computed once
    per batch and shared by the uplink, stride and fastpath cases."""
    cpu = golden_launcher()
    dhcp_tables(cpu)
    want = golden_uplink(cpu, dhcp_frames(n, with_filler))
    return tuple(want), cpu.get_stats()


@pytest.fixture(scope="module")
def dhcp_gpu():
    """One device launcher for all DHCP cases: the DHCP path keeps no
    state but its counters, which the cases read as deltas."""
    gpu = hip_launcher()
    dhcp_tables(gpu)
    return gpu


def stats_delta(after, before):
    return {k: after[k] - before[k] for k in after}


def test_dhcp_shapes_cover_the_issue_list():
    """The generator really produces each request shape and all three
    reply lengths, and one request is longer than its reply."""
    want, st = dhcp_reference(257)
    frames = dhcp_frames(257)
    tx = [(f, w) for f, w in zip(frames, want) if w[0] == TX]
    assert {w[1] for f, w in tx if len(f) == 286} == {322, 328, 332}
    assert any(len(f) > w[1] for f, w in tx)
    assert any(f[12:14] == b"\x81\x00" for f, _ in tx)
    assert any(f[12:14] == b"\x88\xa8" for f, _ in tx)
    assert st["option82_present"] > 0 and st["fastpath_misses"] > 0
    assert st["broadcast_replies"] > 0 and st["unicast_replies"] > 0


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_dhcp_replies_match_golden(shape, dhcp_gpu):
    n, ordered = shape
    frames = dhcp_frames(n)
    want, want_stats = dhcp_reference(n)
    before = dhcp_gpu.get_stats()
    v, ol, rows = run_uplink(dhcp_gpu, frames, ordered)
    check_rows(frames, want, v, ol, rows)
    assert stats_delta(dhcp_gpu.get_stats(), before) == want_stats


@pytest.mark.parametrize("ordered", [False, True], ids=["plain", "order"])
def test_dhcp_stride_344_mixes_both_builders(ordered, dhcp_gpu):
    """Stride 344 is a multiple of 8, not of 16: odd rows are not 16-B
    aligned and take the byte-wise builder, even rows the wide one."""
    n = 65
    frames = dhcp_frames(n)
    assert max(len(f) for f in frames) <= 344
    want, want_stats = dhcp_reference(n)
    before = dhcp_gpu.get_stats()
    v, ol, rows = run_uplink(dhcp_gpu, frames, ordered, stride=344)
    check_rows(frames, want, v, ol, rows)
    assert stats_delta(dhcp_gpu.get_stats(), before) == want_stats


@pytest.mark.parametrize("n", SIZES)
def test_dhcp_fastpath_kernel_matches_golden(n, dhcp_gpu):
    """The same frames through the stand-alone DHCP kernel, which shares
    the reply builder."""
    frames = dhcp_frames(n, False)
    want, want_stats = dhcp_reference(n, False)
    before = dhcp_gpu.get_stats()
    d, l = device_batch(dhcp_gpu, frames)
    v, ol = dhcp_gpu.dhcp_fastpath(d, l, now_sec=NOW_SEC)
    check_rows(frames, want, v, ol, d.cpu().numpy())
    assert stats_delta(dhcp_gpu.get_stats(), before) == want_stats


# ================================================================ sessions
N_FLOWS = 40


def flow_tables(l, n_subs=N_FLOWS):
    for k in range(n_subs):
        ps = 1024 + k * 512
        l.add_subscriber_nat(sub_ip(k), ip2u32("203.0.113.1") + k % 4,
                             ps, ps + 511, subscriber_id=k + 1)


def flow_frame(k, i=0):
    """Packet i of subscriber k's one flow; protocols and lengths vary, so
    the TCP checksum outside the register window and the byte parser
    (42-byte frames) are covered."""
    proto = (17, 6, 17, 1)[k % 4]
    return build_ipv4(sub_mac(k), SERVER_MAC, sub_ip(k), DST, proto=proto,
                      sport=20000 + k, dport=443, icmp_id=700 + k,
                      payload=b"\x00" * ((k % 5) * 7))


def session_table(gpu, inbound=False):
    """{tuple: (nat_ip, nat_port, last_seen, created, pkts_out, bytes_out)}
    from the raw device table, packed accounting deltas folded in; with
    inbound, each row goes on with (state, pkts_in, bytes_in)."""
    arr = gpu.sessions.cpu().numpy().view(
        [("sig", "<u8"), ("src_ip", "<u4"), ("dst_ip", "<u4"),
         ("src_port", "<u2"), ("dst_port", "<u2"), ("protocol", "u1"),
         ("_kp", "3u1"), ("nat_ip", "<u4"), ("nat_port", "<u2"),
         ("orig_port", "<u2"), ("orig_ip", "<u4"), ("state", "u1"),
         ("is_hairpin", "u1"), ("ready", "u1"), ("_p", "u1"),
         ("last_seen", "<u8"), ("created", "<u8"), ("packets_out", "<u8"),
         ("packets_in", "<u8"), ("bytes_out", "<u8"), ("bytes_in", "<u8"),
         ("acct_out", "<u8"), ("acct_in", "<u8"), ("_pad", "3u8")])
    live = arr[(arr["sig"] != 0) & (arr["sig"] != 0xFFFFFFFFFFFFFFFF)]
    out = {}
    for e in live:
        assert e["ready"] == 1
        key = (int(e["src_ip"]), int(e["dst_ip"]), int(e["src_port"]),
               int(e["dst_port"]), int(e["protocol"]))
        assert key not in out, "duplicate session"
        acct = int(e["acct_out"])
        out[key] = (int(e["nat_ip"]), int(e["nat_port"]),
                    int(e["last_seen"]), int(e["created"]),
                    int(e["packets_out"]) + (acct & 0xFFFFFF),
                    int(e["bytes_out"]) + (acct >> 24))
        if inbound:
            acct = int(e["acct_in"])
            out[key] += (int(e["state"]),
                         int(e["packets_in"]) + (acct & 0xFFFFFF),
                         int(e["bytes_in"]) + (acct >> 24))
    return out


def golden_session_table(cpu, inbound=False):
    return {k: (s.nat_ip, s.nat_port, s.last_seen, s.created, s.packets_out,
                s.bytes_out) +
            ((s.state, s.packets_in, s.bytes_in) if inbound else ())
            for k, s in cpu.dp.nat_sessions.items()}


def sorted_export(l):
    recs = l.export_nat_sessions()
    return sorted(map(tuple, recs.tolist()))


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_sessions_create_then_hit(shape):
    """~40 flows in a 64-slot session table: a launch that creates the
    sessions (repeats of a flow wait for its creator), then one that hits
    them, on and past the first slot of their chains."""
    n, ordered = shape
    gpu, cpu = make_pair(sess_log2=6)
    for l in (gpu, cpu):
        flow_tables(l)
    frames = [flow_frame(i % N_FLOWS) for i in range(n)]
    for launch, now in ((1, NOW_NS), (2, NOW_NS + MS)):
        v, ol, rows = run_uplink(gpu, frames, ordered, now_ns=now)
        want = golden_uplink(cpu, frames, now_ns=now)
        check_rows(frames, want, v, ol, rows)
        assert all_stats(gpu) == all_stats(cpu), f"launch {launch}"
        assert session_table(gpu) == golden_session_table(cpu)
        assert sorted_export(gpu) == sorted_export(cpu)
    assert cpu.nat_get_stats()["sessions_created"] == min(n, N_FLOWS)
    if n >= N_FLOWS:
        # the table is loaded enough for chains longer than one slot
        arr = gpu.sessions.cpu().numpy().view("<u8").reshape(64, 16)
        home = arr[:, 0] & np.uint64(63)
        used = arr[:, 0] != 0
        assert (home[used] != np.nonzero(used)[0]).any()


@pytest.mark.parametrize("ordered", [False, True], ids=["plain", "order"])
def test_one_flow_64_times_in_the_creating_batch(ordered):
    gpu, cpu = make_pair(sess_log2=6)
    for l in (gpu, cpu):
        flow_tables(l, 2)
    frames = [flow_frame(0)] * 64 + [flow_frame(1)]
    for now in (NOW_NS, NOW_NS + MS):
        v, ol, rows = run_uplink(gpu, frames, ordered, now_ns=now)
        want = golden_uplink(cpu, frames, now_ns=now)
        check_rows(frames, want, v, ol, rows)
        assert all_stats(gpu) == all_stats(cpu)
        assert session_table(gpu) == golden_session_table(cpu)
    assert cpu.nat_get_stats()["sessions_created"] == 2


def test_flow_recreated_over_a_tombstone_in_its_first_slot():
    """Flow 0 is created in an empty table, so it sits in the first slot of
    its chain; a sweep expires it.  When the flow comes back its first slot
    holds a tombstone, which the snapshot must not take for a hit and the
    claim scan reclaims."""
    gpu, cpu = make_pair(sess_log2=6)
    for l in (gpu, cpu):
        flow_tables(l, 4)
    first = [flow_frame(0)]
    v, ol, rows = run_uplink(gpu, first, False)
    check_rows(first, golden_uplink(cpu, first), v, ol, rows)
    arr = gpu.sessions.cpu().numpy().view("<u8").reshape(64, 16)
    slot = int(np.nonzero(arr[:, 0])[0][0])
    assert int(arr[slot, 0]) & 63 == slot          # in its first slot
    later = NOW_NS + 200 * 10**9                   # > UDP timeout
    for l in (gpu, cpu):
        l.sweep_nat(now_ns=later)
    arr = gpu.sessions.cpu().numpy().view("<u8").reshape(64, 16)
    assert int(arr[slot, 0]) == 0xFFFFFFFFFFFFFFFF
    again = [flow_frame(0), flow_frame(2)]
    for now in (later + MS, later + 2 * MS):
        v, ol, rows = run_uplink(gpu, again, False, now_ns=now)
        want = golden_uplink(cpu, again, now_ns=now)
        check_rows(again, want, v, ol, rows)
        assert all_stats(gpu) == all_stats(cpu)
        assert session_table(gpu) == golden_session_table(cpu)
    arr = gpu.sessions.cpu().numpy().view("<u8").reshape(64, 16)
    assert int(arr[slot, 0]) & 63 == slot and \
        int(arr[slot, 0]) != 0xFFFFFFFFFFFFFFFF    # tombstone reclaimed


# ================================================================ bindings
N_BOUND = 40
MODES = [abi.AS_STRICT, abi.AS_LOOSE, abi.AS_LOG_ONLY, abi.AS_DISABLED]
V6_ADDR = bytes.fromhex("20010db8000000000000000000000042")


def binding_tables(l, default_mode):
    l.set_antispoof_config(
        default_mode=default_mode, log_violations=True,
        allowed_ranges=[(ip2u32("10.1.0.0"), 0xFFFF0000)])
    for k in range(N_BOUND):
        mode = MODES[k % 4]
        # every fifth binding has no IPv4 address: loose mode then checks
        # the allowed ranges, the others find nothing to compare
        l.add_binding(sub_mac(k), ipv4=0 if k % 5 == 4 else sub_ip(k),
                      ipv6=V6_ADDR if k % 7 == 0 else b"", mode=mode)


def v6_frame(mac, src):
    return (SERVER_MAC + mac + b"\x86\xdd" +
            struct.pack(">IHBB", 0x60000000, 8, 17, 64) + src + V6_ADDR +
            b"\x00" * 8)


def binding_frame(i):
    k = i % (N_BOUND + 8)
    mac = sub_mac(k) if k < N_BOUND else (0xEE00000000 + k).to_bytes(6, "big")
    if i % 50 == 7:
        return v6_frame(sub_mac(28), V6_ADDR)     # strict, bound v6: allowed
    if i % 50 == 14:
        return v6_frame(sub_mac(0), bytes(16))    # strict, wrong source
    if i % 50 == 21:
        return v6_frame(sub_mac(14), bytes(16))   # log-only, wrong source
    src = (sub_ip(k), SPOOF_SRC, ip2u32("10.1.77.7"))[i % 3]
    # 42-byte frames take the byte parser, longer ones the vector parser
    return build_ipv4(mac, SERVER_MAC, src, DST, proto=17, sport=1000 + i,
                      dport=53, payload=b"\x00" * (0 if i % 4 == 1 else 22))


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_binding_modes_match_golden(shape):
    """Strict, loose, log-only and disabled bindings in a 64-slot table,
    unknown MACs under each default mode (it cycles with the shape), with
    and without a bound IPv4 address, and IPv6 frames."""
    n, ordered = shape
    default_mode = MODES[SHAPES.index(shape) % 4]
    gpu, cpu = make_pair(binding_log2=6)
    for l in (gpu, cpu):
        binding_tables(l, default_mode)
    frames = [binding_frame(i) for i in range(n)]
    v, ol, rows = run_uplink(gpu, frames, ordered)
    want = golden_uplink(cpu, frames)
    check_rows(frames, want, v, ol, rows)
    assert all_stats(gpu) == all_stats(cpu)
    ev_gpu, ev_cpu = gpu.drain_spoof_events(), cpu.drain_spoof_events()
    assert len(ev_gpu) == len(ev_cpu)
    if n >= 257:
        st = cpu.antispoof_get_stats()
        assert st["packets_dropped"] > 0 and st["packets_logged"] > 0
        assert st["ipv6_violations"] > 0 and st["packets_allowed"] > 0


@pytest.mark.parametrize("default_mode", MODES)
def test_unknown_mac_under_each_default_mode(default_mode):
    gpu, cpu = make_pair(binding_log2=6)
    for l in (gpu, cpu):
        binding_tables(l, default_mode)
    frames = [build_ipv4((0xEE1100000000 + i).to_bytes(6, "big"), SERVER_MAC,
                         (ip2u32("10.1.5.5"), SPOOF_SRC)[i % 2], DST,
                         proto=17, sport=4000 + i, dport=53,
                         payload=b"\x00" * 22) for i in range(65)]
    v, ol, rows = run_uplink(gpu, frames, False)
    check_rows(frames, golden_uplink(cpu, frames), v, ol, rows)
    assert all_stats(gpu) == all_stats(cpu)


# ===================================================== subscriber contexts
N_CTX = 40
DRY = 3            # the subscriber whose bucket runs dry
CTX_LEN = 64       # every context frame is 64 bytes


def ctx_kind(k):
    """(nat_valid, qos): qos None = no policy, else (rate, burst)."""
    if k == DRY:
        return True, (8000, 3 * CTX_LEN + 10)     # three packets, then dry
    return ((True, (0, 0)),                       # rate 0: unlimited
            (True, None),                         # NAT only
            (False, (10**9, 1 << 20)),            # QoS only: NAT passes
            (True, (10**9, 1 << 20)),
            (False, None))[k % 5]                 # no context at all


def ctx_tables(l):
    for k in range(N_CTX):
        nat, qos = ctx_kind(k)
        if nat:
            ps = 1024 + k * 512
            l.add_subscriber_nat(sub_ip(k), ip2u32("203.0.113.9"), ps,
                                 ps + 511, subscriber_id=k + 1)
        if qos is not None:
            l.set_qos_policy(sub_ip(k), qos[0], qos[1], direction="ingress",
                             now_ns=NOW_NS)


def ctx_frame(i):
    k = DRY if i % 8 == 3 else i % N_CTX
    return build_ipv4(sub_mac(k), SERVER_MAC, sub_ip(k), DST, proto=17,
                      sport=20000 + k, dport=53, payload=b"\x00" * 22)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_subscriber_contexts_match_golden(shape):
    """nat_valid and qos_valid each 0 and 1, rate 0, no context, in a
    64-slot table; from n = 63 on one bucket holds three packets and gets
    eight or more, so it runs dry inside the batch: the later packets take
    the refill path (1 ms at 1000 B/s credits one byte) and drop.  Which of
    that flow's identical packets pass depends on thread order, so their
    verdicts are compared as a multiset; their bytes are compared exactly,
    and the second launch drops all of them."""
    n, ordered = shape
    gpu, cpu = make_pair(subnat_log2=6)
    for l in (gpu, cpu):
        ctx_tables(l)
    frames = [ctx_frame(i) for i in range(n)]
    assert all(len(f) == CTX_LEN for f in frames)
    dry_rows = [i for i in range(n) if i % 8 == 3]
    for launch, now in ((1, NOW_NS + MS), (2, NOW_NS + 2 * MS)):
        v, ol, rows = run_uplink(gpu, frames, ordered, now_ns=now)
        want = golden_uplink(cpu, frames, now_ns=now)
        check_rows(frames, want, v, ol, rows, any_order_rows=dry_rows)
        assert all_stats(gpu) == all_stats(cpu), f"launch {launch}"
        assert session_table(gpu) == golden_session_table(cpu)
    if n >= 63:
        st = cpu.qos_get_stats()
        assert st["packets_dropped"] == 2 * len(dry_rows) - 3
        assert cpu.nat_get_stats()["packets_passed"] > 0
