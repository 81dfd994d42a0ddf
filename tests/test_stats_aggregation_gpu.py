"""Block-aggregated stat counters of the batched packet kernels.

The six batched packet kernels add their counters into a per-block
shared array and commit once per block after the grid-stride loop.  The
counters are integers, so every check here is EXACT equality with the
golden model's counters for the same frames — after one launch and again
after a second launch on the same launcher (catches shared memory that is
not re-zeroed, and double commits).

Shapes: batch sizes around the wave (64) and block (256) edges, and a
forced 2-block grid at n = 2*512 + 37 — three grid-stride iterations with
a ragged last wave and a block whose last iteration is empty.  Tables are
small and every batch carries at most one flow per subscriber, so NAT
port allocation is deterministic.
"""
import functools
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import FWD, PASS
from bng_amd.dataplane.packets import (DHCP_DISCOVER, DHCP_REQUEST,
                                       build_dhcp_request, build_ipv4, ip2u32)

NOW_SEC = 1_700_000_000
NOW_NS = NOW_SEC * 10**9
SERVER_MAC = "02:00:00:00:00:01"
DST = ip2u32("93.184.216.34")
SPOOF_SRC = ip2u32("66.6.6.6")

FORCED_CAP = 2                       # blocks
FORCED_N = FORCED_CAP * 256 * 2 + 37  # 1061: 3 iterations, ragged tail
EDGE_SIZES = [1, 63, 64, 65, 255, 256, 257]
# (n, grid cap); cap 0 = built-in default
SHAPES = [(n, 0) for n in EDGE_SIZES] + [(FORCED_N, FORCED_CAP)]
STAGE_SHAPES = [(65, 0), (FORCED_N, FORCED_CAP)]


def shape_id(s):
    return f"n{s[0]}-cap{s[1]}"


# ------------------------------------------------------------ subscribers
def sub_mac(k):
    return (0xAABBCC000000 + k).to_bytes(6, "big")


def sub_ip(k):
    return ip2u32("10.1.0.1") + k


def has_nat(k):
    return k % 11 != 5          # the others hit the NAT "passed" counter


def qos_drops(k):
    return k % 9 == 4           # 10-byte bucket, no refill: always drops


def make_pair(n_subs, egress_qos=False):
    """(HipLauncher, GoldenLauncher) with identical small tables."""
    from bng_amd.dataplane.launcher import GoldenLauncher, HipLauncher
    gpu = HipLauncher(sub_log2=13, sess_log2=13, eim_log2=13, subnat_log2=13,
                      qos_log2=13, binding_log2=13, n_pools=16)
    cpu = GoldenLauncher()
    cpu.dp.now_ns = NOW_NS
    for l in (gpu, cpu):
        l.set_server_config(bytes.fromhex("020000000001"),
                            ip2u32("10.255.255.1"))
        l.add_pool(1, ip2u32("10.1.0.0"), 16, ip2u32("10.1.255.254"),
                   ip2u32("8.8.8.8"), ip2u32("1.1.1.1"), 3600)
        l.set_antispoof_config(default_mode=abi.AS_DISABLED,
                               log_violations=True)
        for k in range(n_subs):
            ip = sub_ip(k)
            l.add_subscriber(sub_mac(k), 1, ip, NOW_SEC + 600)
            if has_nat(k):
                ps = 1024 + (k % 100) * 512
                l.add_subscriber_nat(ip, ip2u32("203.0.113.1") + k // 100,
                                     ps, ps + 511, subscriber_id=k + 1)
            if qos_drops(k):
                l.set_qos_policy(ip, 8000, 10, direction="ingress",
                                 now_ns=NOW_NS)
            else:
                l.set_qos_policy(ip, 0, 0, direction="ingress",
                                 now_ns=NOW_NS)
            if egress_qos:
                l.set_qos_policy(ip, 0, 0, direction="egress",
                                 now_ns=NOW_NS)
            l.add_binding(sub_mac(k), ipv4=ip, mode=abi.AS_STRICT)
    return gpu, cpu


# ----------------------------------------------------------------- frames
def f_data(k, src=None):
    # payload 0..28 B: 42-byte frames take the byte parser, >= 48 the
    # vector parser; lengths differ so the byte sums are not trivial
    return build_ipv4(sub_mac(k), SERVER_MAC, sub_ip(k) if src is None
                      else src, DST, proto=17, sport=20000 + k, dport=53,
                      payload=b"\x00" * ((k % 5) * 7))


def f_dataish(k):
    """data frame; every 7th is spoofed (strict binding -> DROP+log)."""
    return f_data(k, SPOOF_SRC) if k % 7 == 3 else f_data(k)


def f_dhcp(k):
    mac = sub_mac(k) if k % 13 != 6 else (0xEE0000000000 + k).to_bytes(
        6, "big")                    # unknown client -> fastpath miss
    return build_dhcp_request(mac, DHCP_DISCOVER if k % 2 else DHCP_REQUEST,
                              xid=0x1000 + k)


def f_hostpass(k):
    """PPPoE discovery / PPPoE session / ARP: the uplink `continue` path."""
    et = (0x8863, 0x8864, 0x0806)[k % 3]
    return (bytes.fromhex("020000000001") + sub_mac(k) +
            struct.pack(">H", et) + b"\x11" * 28)


def f_truncated(k):
    """10 B (no Ethernet header) or 20 B (IPv4 ethertype, cut header)."""
    return f_data(k)[:10 if k % 2 else 20]


@functools.lru_cache(maxsize=None)
def mix_frames(mix, n):
    if mix == "data":
        return tuple(f_dataish(k) for k in range(n))
    if mix == "dhcp":
        return tuple(f_dhcp(k) for k in range(n))
    if mix in ("mixed", "mixed_sorted"):
        return tuple(f_dhcp(k) if k % 10 == 9 else f_dataish(k)
                     for k in range(n))
    if mix == "passthru":
        kinds = (f_hostpass, f_truncated, f_dataish, f_dhcp)
        return tuple(kinds[k % 4](k) for k in range(n))
    raise ValueError(mix)


def is_dhcp(f):
    return (len(f) >= 42 and f[12:14] == b"\x08\x00" and f[14] == 0x45 and
            f[23] == 17 and f[36:38] == b"\x00\x43")


# ----------------------------------------------------------- golden chain
def golden_uplink(cpu, frames):
    """The fused uplink kernel's dispatch, on the golden model."""
    verdicts = []
    for f in frames:
        cpu.dp.now_ns = NOW_NS
        et = struct.unpack_from(">H", f, 12)[0] if len(f) >= 14 else 0
        if et in (0x8863, 0x8864, 0x0806):
            verdicts.append(PASS)
        elif is_dhcp(f):
            verdicts.append(cpu.dp.dhcp_fastpath(bytearray(f))[0])
        else:
            fb = bytearray(f)
            v = cpu.dp.antispoof(bytes(fb))
            if v == FWD:
                v = cpu.dp.nat44_egress(fb)
            if v == FWD:
                # ingress QoS is keyed by the subscriber's own address:
                # the kernel reuses the context entry it probed before
                # SNAT rewrote the source, so the model gets the original
                v = cpu.dp.qos(bytes(f), "ingress")
            verdicts.append(v)
    return verdicts


def all_stats(l):
    return {"dhcp": l.get_stats(), "nat": l.nat_get_stats(),
            "qos": l.qos_get_stats(), "antispoof": l.antispoof_get_stats()}


@pytest.fixture
def grid_cap():
    """Setter for the packet-kernel grid cap; always restored to default."""
    from bng_amd.dataplane.build import get_ext
    ext = get_ext(required=True)
    try:
        yield ext.set_pkt_grid_cap
    finally:
        ext.set_pkt_grid_cap(0)


# ------------------------------------------------------------------ tests
def test_grid_cap_setter_roundtrip(grid_cap):
    from bng_amd.dataplane.build import get_ext
    ext = get_ext(required=True)
    default = ext.get_pkt_grid_cap()
    assert default > 0
    grid_cap(FORCED_CAP)
    assert ext.get_pkt_grid_cap() == FORCED_CAP
    grid_cap(0)
    assert ext.get_pkt_grid_cap() == default


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("mix", ["data", "dhcp", "mixed", "mixed_sorted",
                                 "passthru"])
def test_uplink_counters_match_golden(mix, shape, grid_cap):
    import torch
    n, cap = shape
    frames = mix_frames(mix, n)
    gpu, cpu = make_pair(n)
    grid_cap(cap)
    order = None
    if mix == "mixed_sorted":
        cls = np.array([1 if is_dhcp(f) else 0 for f in frames])
        order = torch.from_numpy(
            np.argsort(cls, kind="stable").astype(np.int32)).to(gpu.device)
    for launch in (1, 2):
        # a fresh copy of the frames: DHCP replies are built in place
        data, lens = gpu.make_batch(list(frames))
        v, _ = gpu.uplink(data, lens, now_ns=NOW_NS, now_sec=NOW_SEC,
                          order=order)
        vc = golden_uplink(cpu, frames)
        assert v.cpu().tolist() == vc, f"verdicts differ (launch {launch})"
        got, want = all_stats(gpu), all_stats(cpu)
        print(f"launch {launch}: {got}")
        assert got == want, f"counters differ after launch {launch}"
    if n >= 64 and mix in ("mixed", "passthru"):
        # the mixes really exercise every counter group
        assert want["dhcp"]["fastpath_hits"] > 0
        assert want["nat"]["packets_snat"] > 0
        assert want["qos"]["bytes_passed"] > 0
        assert want["antispoof"]["packets_dropped"] > 0


@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=shape_id)
def test_nat44_counters_match_golden(shape, grid_cap):
    n, cap = shape
    frames = [f_data(k) for k in range(n)]
    gpu, cpu = make_pair(n)
    grid_cap(cap)
    for launch in (1, 2):
        data, lens = gpu.make_batch(frames, stride=128)
        v = gpu.nat44(data, lens, egress=True, now_ns=NOW_NS)
        res = cpu.process_nat44(frames, egress=True, now_ns=NOW_NS)
        assert v.cpu().tolist() == [r[0] for r in res]
        print(f"launch {launch}: {gpu.nat_get_stats()}")
        assert gpu.nat_get_stats() == cpu.nat_get_stats()
    assert cpu.nat_get_stats()["packets_snat"] > 0


@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=shape_id)
def test_qos_counters_match_golden(shape, grid_cap):
    n, cap = shape
    frames = [f_data(k) for k in range(n)]
    gpu, cpu = make_pair(n)
    grid_cap(cap)
    for launch in (1, 2):
        data, lens = gpu.make_batch(frames, stride=128)
        v = gpu.qos(data, lens, egress=False, now_ns=NOW_NS)
        cpu.dp.now_ns = NOW_NS
        assert v.cpu().tolist() == [cpu.dp.qos(f, "ingress") for f in frames]
        print(f"launch {launch}: {gpu.qos_get_stats()}")
        assert gpu.qos_get_stats() == cpu.qos_get_stats()
    st = cpu.qos_get_stats()
    assert st["bytes_passed"] > 0 and st["bytes_dropped"] > 0


@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=shape_id)
def test_antispoof_counters_match_golden(shape, grid_cap):
    n, cap = shape
    frames = [f_dataish(k) for k in range(n)]
    gpu, cpu = make_pair(n)
    grid_cap(cap)
    for launch in (1, 2):
        data, lens = gpu.make_batch(frames, stride=128)
        v = gpu.antispoof(data, lens, now_ns=NOW_NS)
        assert v.cpu().tolist() == [cpu.dp.antispoof(f) for f in frames]
        print(f"launch {launch}: {gpu.antispoof_get_stats()}")
        assert gpu.antispoof_get_stats() == cpu.antispoof_get_stats()
    st = cpu.antispoof_get_stats()
    assert st["packets_allowed"] > 0 and st["packets_dropped"] > 0
    assert st["packets_logged"] > 0


@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=shape_id)
def test_dhcp_fastpath_counters_match_golden(shape, grid_cap):
    n, cap = shape
    frames = [f_dhcp(k) for k in range(n)]
    gpu, cpu = make_pair(n)
    grid_cap(cap)
    for launch in (1, 2):
        data, lens = gpu.make_batch(frames)
        v, _ = gpu.dhcp_fastpath(data, lens, now_sec=NOW_SEC)
        res = cpu.process_dhcp(frames, now_sec=NOW_SEC)
        assert v.cpu().tolist() == [r[0] for r in res]
        print(f"launch {launch}: {gpu.get_stats()}")
        assert gpu.get_stats() == cpu.get_stats()
    st = cpu.get_stats()
    assert st["fastpath_hits"] > 0 and st["fastpath_misses"] > 0


def test_downlink_counters_match_golden(grid_cap):
    """Return path at the forced 2-block shape: DNAT + egress QoS."""
    n = FORCED_N
    subs = [k for k in range(n + n // 8) if has_nat(k)][:n]
    assert len(subs) == n
    gpu, cpu = make_pair(subs[-1] + 1, egress_qos=True)
    out = [f_data(k) for k in subs]
    data, lens = gpu.make_batch(out, stride=128)
    v = gpu.nat44(data, lens, egress=True, now_ns=NOW_NS)
    assert v.cpu().tolist() == [FWD] * n
    cpu.process_nat44(out, egress=True, now_ns=NOW_NS)
    host = data.cpu().numpy()
    back = []
    for i in range(n):
        nat_ip = struct.unpack_from(">I", host[i], 26)[0]
        nat_port = struct.unpack_from(">H", host[i], 34)[0]
        back.append(build_ipv4(SERVER_MAC, "02:00:00:00:00:02", DST, nat_ip,
                               proto=17, sport=53, dport=nat_port,
                               payload=b"\x00" * ((i % 5) * 7)))
    grid_cap(FORCED_CAP)
    for launch in (1, 2):
        d2, l2 = gpu.make_batch(back, stride=128)
        v = gpu.downlink(d2, l2, now_ns=NOW_NS)
        vc = []
        for f in back:
            fb = bytearray(f)
            cpu.dp.now_ns = NOW_NS
            x = cpu.dp.nat44_ingress(fb)
            if x == FWD:
                x = cpu.dp.qos(bytes(fb), "egress")
            vc.append(x)
        assert v.cpu().tolist() == vc
        got = (gpu.nat_get_stats(), gpu.qos_get_stats())
        print(f"launch {launch}: {got}")
        assert got == (cpu.nat_get_stats(), cpu.qos_get_stats())
    assert cpu.nat_get_stats()["packets_dnat"] == 2 * n
    assert cpu.qos_get_stats()["packets_passed"] == 2 * n
