"""Per-subscriber traffic accounting on the device: acct_resolve_kernel and
acct_commit_kernel around the uplink pipeline, acct_downlink_kernel behind
the downlink pipeline, and the entry CRUD kernels.

The counters are integers, so every comparison with the golden model is
EXACT equality, entry by entry and field by field.  That needs verdicts
that do not depend on lane order, and the inputs are chosen for it: QoS
buckets are unlimited or the 10-byte, no-refill kind that always drops,
NATed subscribers carry one flow each, and the cases that put many packets
of one subscriber into a batch use subscribers without a port block.  Each
differential test first asserts GPU verdicts == golden verdicts for every
packet, and — wherever the case holds both kinds — that some entry
forwarded and some entry dropped, so it cannot pass on all-zero tables.

Shapes: batch sizes around the wave (64) and block (256) edges, and a
forced 2-block grid at n = 2*256*2 + 37 — three grid-stride iterations
with a ragged last wave.  Tables are small (acct_log2 4..13), stride 128.
"""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import DROP, FWD, PASS, TX
from bng_amd.dataplane.packets import (DHCP_DISCOVER, build_dhcp_request,
                                       build_ipv4, ip2u32)
from bng_amd.pppoe import codec as C

NOW_SEC = 1_700_000_000
NOW_NS = NOW_SEC * 10**9
NOW2_NS = NOW_NS + 1000              # the downlink batches' clock
SERVER_MAC = bytes.fromhex("020000000001")
CORE_MAC = bytes.fromhex("020000000002")
DST = ip2u32("93.184.216.34")
STRIDE = 128

FORCED_CAP = 2
FORCED_N = FORCED_CAP * 256 * 2 + 37        # 1061
EDGE_SIZES = [1, 63, 64, 65, 255, 256, 257]
SHAPES = [(n, 0) for n in EDGE_SIZES] + [(FORCED_N, FORCED_CAP)]
LANE_SHAPES = [(64, 0), (65, 0), (FORCED_N, FORCED_CAP)]
DTYPE = np.dtype(abi.ACCT_ENTRY_DTYPE)


def shape_id(s):
    return f"n{s[0]}-cap{s[1]}"


def sub_mac(k):
    return (0xAABBCC000000 + k).to_bytes(6, "big")


PUB = 5000          # subscribers from this index on have public addresses


def sub_ip(k):
    if k >= PUB:
        # NAT leaves a public source alone (FWD); a private one without a
        # port block would go to the host (PASS) and count nothing
        return ip2u32("198.51.100.1") + (k - PUB)
    return ip2u32("10.1.0.1") + k


def qos_drops(k):
    return k % 9 == 4           # 10-byte bucket, no refill: always drops


def accounted(k):
    return k % 4 != 3


def make_pair(n_subs, has_nat=lambda j: True, egress_drop=(),
              acct=accounted, first=0, **kw):
    """(HipLauncher, GoldenLauncher) with identical small tables holding
    subscribers first .. first + n_subs - 1; the predicates take the index
    relative to `first`, and the subscribers `acct` selects are accounted
    on both."""
    from bng_amd.dataplane.launcher import GoldenLauncher, HipLauncher
    gpu = HipLauncher(sub_log2=13, sess_log2=13, eim_log2=13, subnat_log2=13,
                      qos_log2=13, binding_log2=13, n_pools=16,
                      pppoe_log2=13, acct_log2=kw.pop("acct_log2", 13))
    cpu = GoldenLauncher()
    cpu.dp.now_ns = NOW_NS
    for l in (gpu, cpu):
        l.set_server_config(SERVER_MAC, ip2u32("10.255.255.1"))
        l.add_pool(1, ip2u32("10.1.0.0"), 16, ip2u32("10.1.255.254"),
                   ip2u32("8.8.8.8"), ip2u32("1.1.1.1"), 3600)
        l.set_antispoof_config(default_mode=abi.AS_DISABLED,
                               log_violations=True)
        for j in range(n_subs):
            k = first + j
            ip = sub_ip(k)
            l.add_subscriber(sub_mac(k), 1, ip, NOW_SEC + 600)
            if has_nat(j):
                ps = 1024 + (j % 100) * 512
                l.add_subscriber_nat(ip, ip2u32("203.0.113.1") + j // 100,
                                     ps, ps + 511, subscriber_id=j + 1)
            if qos_drops(j):
                l.set_qos_policy(ip, 8000, 10, direction="ingress",
                                 now_ns=NOW_NS)
            else:
                l.set_qos_policy(ip, 0, 0, direction="ingress",
                                 now_ns=NOW_NS)
            if j in egress_drop:
                l.set_qos_policy(ip, 8000, 10, direction="egress",
                                 now_ns=NOW_NS)
            l.add_binding(sub_mac(k), ipv4=ip, mode=abi.AS_STRICT)
        ips = [sub_ip(first + j) for j in range(n_subs) if acct(j)]
        if ips:
            l.acct_add(ips)                  # one launch
    return gpu, cpu


@pytest.fixture
def grid_cap():
    from bng_amd.dataplane.build import get_ext
    ext = get_ext(required=True)
    try:
        yield ext.set_pkt_grid_cap
    finally:
        ext.set_pkt_grid_cap(0)


@pytest.fixture
def combine():
    """Setter for the commit's peel-round count; always restored."""
    from bng_amd.dataplane.build import get_ext
    ext = get_ext(required=True)
    default = ext.get_acct_combine()
    try:
        yield ext.set_acct_combine
    finally:
        ext.set_acct_combine(default)


# ----------------------------------------------------------------- frames
def f_data(k, length, mac=None, sport=None):
    """UDP data frame of subscriber k, `length` bytes on the wire."""
    f = build_ipv4(sub_mac(k) if mac is None else mac, SERVER_MAC, sub_ip(k),
                   DST, proto=17, sport=20000 + k if sport is None else sport,
                   dport=53, payload=bytes(length - 42))
    assert len(f) == length
    return f


def mixed_len(i):
    return 60 + (i * 7) % 61                 # 60..120


def mix_frame(i):
    """One flow per subscriber i, with the frames that must count nothing
    strewn in."""
    if i % 10 == 9:
        return build_dhcp_request(sub_mac(i), DHCP_DISCOVER, xid=0x1000 + i)
    if i % 32 == 3:
        return SERVER_MAC + sub_mac(i) + b"\x08\x06" + bytes(28)     # ARP
    if i % 32 == 5:                          # VLAN-tagged data frame
        f = f_data(i, mixed_len(i))
        return f[:12] + b"\x81\x00\x00\x64" + f[12:]
    return f_data(i, mixed_len(i))


def is_dhcp(f):
    return (len(f) >= 42 and f[12:14] == b"\x08\x00" and f[14] == 0x45 and
            f[23] == 17 and f[36:38] == b"\x00\x43")


# ----------------------------------------------------------- golden chain
def golden_uplink(cpu, frames, now_ns=NOW_NS, stride=STRIDE):
    """HipLauncher.uplink's sequence on the golden model: decap, resolve,
    the fused kernel's dispatch, REJECT -> DROP, commit.  A frame longer
    than the row is cut to it, as make_batch does.  Returns the verdicts."""
    dp = cpu.dp
    verdicts = []
    for f in frames:
        dp.now_ns = now_ns
        f = f[:stride]
        fb = bytearray(f)
        st, L = dp.pppoe_decap(fb) if dp.pppoe_sessions \
            else (abi.PPPOE_NONE, len(f))
        g = bytes(fb[:L]) if st == abi.PPPOE_DECAP else f
        key = dp.acct_resolve(g, "src")
        out_len = len(g)
        et = struct.unpack_from(">H", g, 12)[0] if len(g) >= 14 else 0
        if et in (0x8863, 0x8864, 0x0806):
            v = PASS
        elif is_dhcp(g):
            v, out_len = dp.dhcp_fastpath(bytearray(g))
        else:
            fb = bytearray(g)
            v = dp.antispoof(bytes(fb))
            if v == FWD:
                v = dp.nat44_egress(fb)
            if v == FWD:
                # ingress QoS is keyed by the subscriber's own address
                v = dp.qos(g, "ingress")
        if st == abi.PPPOE_REJECT:
            v = DROP
        dp.acct_commit(key, "uplink", out_len, v, now_ns)
        verdicts.append(v)
    return verdicts


def golden_downlink(cpu, frames, now_ns=NOW2_NS):
    dp = cpu.dp
    verdicts = []
    for f in frames:
        dp.now_ns = now_ns
        fb = bytearray(f)
        v = dp.nat44_ingress(fb)
        if v == FWD:
            v = dp.qos(bytes(fb), "egress")
        dp.acct_commit(dp.acct_resolve(fb, "dst"), "downlink", len(fb), v,
                       now_ns)
        if dp.pppoe_sessions:
            _st, v, _L = dp.pppoe_encap(fb, v, STRIDE)
        verdicts.append(v)
    return verdicts


def rows(arr):
    return [tuple(int(x) for x in r) for r in arr]


def assert_entries_equal(gpu, cpu, ips, what=""):
    got, want = gpu.acct_read(ips), cpu.acct_read(ips)
    assert got.dtype == DTYPE and want.dtype == DTYPE
    for ip, g, w in zip(ips, rows(got), rows(want)):
        assert g == w, f"{what}: entry of {ip:#x}: gpu {g} golden {w}"
    return want


def assert_not_trivial(want, direction="up"):
    assert (want[f"{direction}_pkts"] > 0).any()
    assert (want[f"{direction}_drop_pkts"] > 0).any()


def run_uplink(gpu, cpu, frames, what, stride=STRIDE, **kw):
    """One batch through both; asserts the verdicts agree packet by packet.
    Returns (verdicts, the batch's rows after the pipeline)."""
    data, lens = gpu.make_batch(list(frames), stride=stride)
    v, _ = gpu.uplink(data, lens, now_ns=NOW_NS, now_sec=NOW_SEC, **kw)
    vc = golden_uplink(cpu, frames, stride=stride)
    assert v.cpu().tolist() == vc, f"{what}: verdicts differ"
    return vc, data.cpu().numpy()


def return_frame(row, length):
    """The core's answer to a forwarded (SNAT-ed) UDP frame."""
    nat_ip = struct.unpack_from(">I", row, 26)[0]
    nat_port = struct.unpack_from(">H", row, 34)[0]
    return build_ipv4(CORE_MAC, SERVER_MAC, DST, nat_ip, proto=17, sport=53,
                      dport=nat_port, payload=bytes(length - 42))


# ------------------------------------------------------ uplink differential
# stride 128 cuts the DHCP DISCOVERs short (PASS); the one 512-byte case
# has them answered on the device (TX)
@pytest.mark.parametrize("shape", [s + (STRIDE,) for s in SHAPES] +
                         [(257, 0, 512)],
                         ids=lambda s: f"{shape_id(s)}-stride{s[2]}")
def test_uplink_entries_match_golden(shape, grid_cap):
    n, cap, stride = shape
    frames = [mix_frame(i) for i in range(n)]
    gpu, cpu = make_pair(n)
    grid_cap(cap)
    ips = [sub_ip(k) for k in range(n)]
    for launch in (1, 2):
        # the second batch catches double commits and a stale slot[]
        vc, _ = run_uplink(gpu, cpu, frames, f"launch {launch}",
                           stride=stride)
        want = assert_entries_equal(gpu, cpu, ips, f"launch {launch}")
        print(f"launch {launch}: fwd {int(want['up_pkts'].sum())} pkts "
              f"{int(want['up_bytes'].sum())} B, "
              f"dropped {int(want['up_drop_pkts'].sum())}")
        for k in range(n):
            if not accounted(k):             # reads back as a zero row
                assert rows(want[k:k + 1]) == [(0,) * 8]
    assert gpu.acct_launches == {"resolve": 2, "commit": 2, "downlink": 0}
    if n >= 63:
        assert_not_trivial(want)
        assert {PASS, DROP, FWD} <= set(vc)
        assert (TX in vc) == (stride == 512)
        assert int(want["up_pkts"].sum()) < 2 * vc.count(FWD)  # unaccounted
        live = want[want["up_pkts"] > 0]
        assert (live["last_seen"] == NOW_NS).all()
        assert (want["down_pkts"] == 0).all()
    assert len(gpu.acct_export()) == gpu.acct_count == cpu.acct_count


# ------------------------------------------------- lane distributions
N_LANE_SUBS = 140


def spoofed(k, length):
    """Subscriber k's address from another subscriber's MAC: antispoof
    DROP, billed to k as a dropped packet."""
    return f_data(PUB + k, length, mac=sub_mac(PUB + k + 1))


def lane_one(i):
    return f_data(PUB, 60 + i % 61, sport=1000 + i)


def lane_two(i):
    return f_data(PUB + i % 2, mixed_len(i), sport=1000 + i)


FIVE = [0, 1, 0, 2, 0, 1, 5, 0, 1, 2, 8, 0, 1, 2, 5]   # sizes 5,4,3,2,1


def lane_five_groups(i):
    r = i % 21
    k = FIVE[r] if r < len(FIVE) else 10 + i % 100     # else a singleton
    return f_data(PUB + k, mixed_len(i), sport=1000 + i)


def lane_distinct(i):
    return f_data(PUB + i % 128, mixed_len(i), sport=1000 + i)


def lane_fwd_drop(i):
    k = (0, 1, 4)[i % 3]                     # subscriber 4 QoS-drops as well
    if (i // 3) % 2:
        return spoofed(k, mixed_len(i))
    return f_data(PUB + k, mixed_len(i))


def lane_spanning(i):
    return f_data(PUB + i // 48, mixed_len(i), sport=1000 + i)


LANE_CASES = {"one": lane_one, "two": lane_two, "five_groups":
              lane_five_groups, "distinct": lane_distinct,
              "fwd_drop": lane_fwd_drop, "spanning": lane_spanning}


def lane_pair():
    # no port blocks: many packets of one subscriber in a batch stay
    # order-independent; subscribers 6, 13, ... are not accounted
    return make_pair(N_LANE_SUBS, has_nat=lambda j: False,
                     acct=lambda j: j % 7 != 6, first=PUB)


LANE_IPS = [sub_ip(PUB + k) for k in range(N_LANE_SUBS)]


@pytest.mark.parametrize("shape", LANE_SHAPES, ids=shape_id)
@pytest.mark.parametrize("case", sorted(LANE_CASES))
def test_commit_exact_for_lane_distribution(case, shape, grid_cap):
    n, cap = shape
    frames = [LANE_CASES[case](i) for i in range(n)]
    gpu, cpu = lane_pair()
    grid_cap(cap)
    ips = LANE_IPS
    for launch in (1, 2):
        vc, _ = run_uplink(gpu, cpu, frames, f"{case} launch {launch}")
        want = assert_entries_equal(gpu, cpu, ips, f"{case} launch {launch}")
    assert (want["up_pkts"] > 0).any()
    if case == "one":
        assert int(want[0]["up_pkts"]) == 2 * n
        assert int(want[0]["up_bytes"]) == 2 * sum(len(f) for f in frames)
    if case == "fwd_drop":
        assert_not_trivial(want)
        assert int(want[0]["up_pkts"]) > 0 and \
            int(want[0]["up_drop_pkts"]) > 0          # mixed in one group
    if case == "distinct" and n >= 64:
        assert (want["up_drop_pkts"] > 0).any()       # the QoS droppers
    assert int(want["up_pkts"].sum()) + int(want["up_drop_pkts"].sum()) <= \
        2 * (vc.count(FWD) + vc.count(DROP))


@pytest.mark.parametrize("rounds", [0, 1, 2, -1], ids=lambda r: f"rounds{r}")
@pytest.mark.parametrize("case", ["five_groups", "fwd_drop", "spanning"])
def test_every_combining_variant_is_exact(case, rounds, combine, grid_cap):
    n = 2 * 256 + 37                         # one block, three iterations
    frames = [LANE_CASES[case](i) for i in range(n)]
    gpu, cpu = lane_pair()
    grid_cap(1)
    combine(rounds)
    run_uplink(gpu, cpu, frames, f"{case} rounds {rounds}")
    want = assert_entries_equal(
        gpu, cpu, LANE_IPS, case)
    assert (want["up_pkts"] > 0).any()


# ---------------------------------------------------------- sorted dispatch
def test_sorted_dispatch_gives_identical_entries():
    import torch
    n = 257
    frames = [mix_frame(i) for i in range(n)]
    ips = [sub_ip(k) for k in range(n)]
    rng = np.random.default_rng(7)
    read = []
    for mode in ("plain", "sort", "shuffled"):
        gpu, cpu = make_pair(n)
        kw = {}
        if mode == "sort":
            kw["sort_by_type"] = True
        elif mode == "shuffled":
            kw["order"] = torch.from_numpy(
                rng.permutation(n).astype(np.int32)).to(gpu.device)
        run_uplink(gpu, cpu, frames, mode, **kw)
        want = assert_entries_equal(gpu, cpu, ips, mode)
        read.append(gpu.acct_read(ips))
    assert_not_trivial(want)
    assert rows(read[0]) == rows(read[1]) == rows(read[2])


# ----------------------------------------------------------------- downlink
@pytest.mark.parametrize("shape", [(65, 0), (256 + 37, 1)], ids=shape_id)
def test_downlink_entries_match_golden(shape, grid_cap):
    n, cap = shape
    # subscribers 2 and 10 have an always-drop egress bucket; 2 is accounted
    gpu, cpu = make_pair(n, egress_drop=(2, 10))
    ips = [sub_ip(k) for k in range(n)]
    # uplink first: one flow per subscriber creates the NAT sessions
    up = [f_data(k, mixed_len(k)) for k in range(n)]
    vu, host = run_uplink(gpu, cpu, up, "uplink")
    # SNAT runs ahead of QoS: a QoS-dropped frame made its session too
    assert set(vu) == {FWD, DROP}
    back = [return_frame(host[k], mixed_len(k + 3)) for k in range(n)]
    # a public port nobody holds: whatever the verdict, it counts nothing
    stray = build_ipv4(CORE_MAC, SERVER_MAC, DST, ip2u32("203.0.113.1"),
                       proto=17, sport=53, dport=60001, payload=bytes(30))
    back.insert(len(back) // 2, stray)
    before = cpu.acct_read(ips)
    grid_cap(cap)
    for launch in (1, 2):
        d2, l2 = gpu.make_batch(back, stride=STRIDE)
        v = gpu.downlink(d2, l2, now_ns=NOW2_NS)
        vc = golden_downlink(cpu, back)
        assert v.cpu().tolist() == vc, f"launch {launch}: verdicts differ"
        want = assert_entries_equal(gpu, cpu, ips, f"launch {launch}")
    assert_not_trivial(want, "down")
    assert FWD in vc and DROP in vc
    live = want[want["down_pkts"] > 0]
    assert (live["last_seen"] == NOW2_NS).all()
    # the drop-only and the untouched entries keep the uplink's stamp
    idle = want[(want["down_pkts"] == 0) & (want["up_pkts"] > 0)]
    assert (idle["last_seen"] == NOW_NS).all()
    for f in ("up_bytes", "up_pkts", "up_drop_pkts"):
        assert (want[f] == before[f]).all(), f
    assert int(want["down_pkts"].sum()) < 2 * vc.count(FWD)   # unaccounted
    assert gpu.acct_launches["downlink"] == 2


# -------------------------------------------------------------------- PPPoE
def wrap(frame, sid):
    return C.SessionPacket(sid, C.PROTO_IPV4, frame[14:], src_mac=frame[6:12],
                           dst_mac=frame[0:6]).encode()


def test_pppoe_counts_the_ipoe_length_both_ways():
    sid = 0x0011
    gpu, cpu = make_pair(3, acct=lambda k: True)
    for l in (gpu, cpu):
        l.add_pppoe_session(sid, sub_mac(0), sub_ip(0))
    ips = [sub_ip(k) for k in range(3)]
    twin = f_data(0, 77)
    wire = wrap(twin, sid)
    assert len(wire) == len(twin) + 8
    wrong_mac = bytearray(wrap(f_data(0, 90), sid))
    wrong_mac[6:12] = sub_mac(1)
    up = [wire, bytes(wrong_mac), f_data(1, 64)]
    vc, host = run_uplink(gpu, cpu, up, "uplink")
    assert vc == [FWD, DROP, FWD]
    assert gpu.last_pppoe_state.cpu().tolist() == [
        abi.PPPOE_DECAP, abi.PPPOE_REJECT, abi.PPPOE_NONE]
    want = assert_entries_equal(gpu, cpu, ips, "uplink")
    # 8 less than the wire frame; the rejected frame counts nothing at all
    assert rows(want[["up_bytes", "up_pkts", "up_drop_pkts"]]) == [
        (len(wire) - 8, 1, 0), (64, 1, 0), (0, 0, 0)]

    back = return_frame(host[0], 83)
    d2, l2 = gpu.make_batch([back], stride=STRIDE)
    v = gpu.downlink(d2, l2, now_ns=NOW2_NS)
    assert v.cpu().tolist() == golden_downlink(cpu, [back]) == [FWD]
    assert gpu.last_pppoe_state.cpu().tolist() == [abi.PPPOE_ENCAP]
    assert int(l2.cpu().numpy().view(np.uint16)[0]) == len(back) + 8
    want = assert_entries_equal(gpu, cpu, ips, "downlink")
    # the pre-encap length
    assert rows(want[["down_bytes", "down_pkts"]])[0] == (len(back), 1)
    assert int(want[0]["last_seen"]) == NOW2_NS


# ---------------------------------------------------------- table lifecycle
def colliding_ips(log2, count):
    """`count` addresses whose accounting keys share one home slot."""
    mask = (1 << log2) - 1
    by_slot = {}
    ip = ip2u32("192.0.2.1")           # public: forwards without a port block
    while True:
        s = by_slot.setdefault(abi.mix64(abi.acct_key(ip)) & mask, [])
        s.append(ip)
        if len(s) == count:
            return s
        ip += 1


def plain_launcher(acct_log2):
    """No subscriber tables at all: antispoof disabled, no port block, no
    bucket — every IPv4 frame from a public address forwards unchanged."""
    from bng_amd.dataplane.launcher import HipLauncher
    gpu = HipLauncher(sub_log2=13, sess_log2=13, eim_log2=13, subnat_log2=13,
                      qos_log2=13, binding_log2=13, n_pools=16,
                      pppoe_log2=13, acct_log2=acct_log2)
    gpu.set_server_config(SERVER_MAC, ip2u32("10.255.255.1"))
    return gpu


def frame_from(ip, length):
    return build_ipv4(b"\xaa\xbb\xcc\x00\x00\x01", SERVER_MAC, ip, DST,
                      proto=17, sport=4000, dport=53,
                      payload=bytes(length - 42))


def send_up(gpu, frames):
    data, lens = gpu.make_batch(frames, stride=STRIDE)
    v, _ = gpu.uplink(data, lens, now_ns=NOW_NS, now_sec=NOW_SEC)
    assert v.cpu().tolist() == [FWD] * len(frames)


def counters(row):
    return tuple(int(row[f]) for f in abi.ACCT_COUNTERS)


def test_table_lifecycle_with_tombstones():
    a, b, c = colliding_ips(4, 3)
    gpu = plain_launcher(acct_log2=4)
    gpu.acct_add([a, b, c])
    assert gpu.acct_count == 3
    send_up(gpu, [frame_from(a, 60), frame_from(b, 70), frame_from(c, 80),
                  frame_from(a, 61)])
    r = gpu.acct_read([a, b, c])
    assert [counters(x)[:2] for x in r] == [(121, 2), (70, 1), (80, 1)]
    assert [int(x) for x in r["key"]] == [abi.acct_key(i) for i in (a, b, c)]

    final = gpu.acct_remove([a])
    assert rows(final) == rows(r[:1])        # the pre-removal read
    assert gpu.acct_count == 2 and len(gpu.acct_export()) == 2
    assert rows(gpu.acct_read([a])) == [(0,) * 8]
    # b and c are found behind the tombstone and keep counting; a's traffic
    # counts nothing now
    send_up(gpu, [frame_from(a, 60), frame_from(b, 71), frame_from(c, 81)])
    r = gpu.acct_read([b, c])
    assert [counters(x)[:2] for x in r] == [(141, 2), (161, 2)]

    gpu.acct_add([a])                        # reuses the tombstone, zeroed
    assert counters(gpu.acct_read([a])[0]) == (0,) * 7
    exp = gpu.acct_export()
    assert len(exp) == 3 == gpu.acct_count
    assert sorted(int(k) for k in exp["key"]) == sorted(
        abi.acct_key(i) for i in (a, b, c))
    blob = gpu.acct.cpu().numpy().view(DTYPE)
    assert (blob["key"] == abi.KEY_TOMBSTONE).sum() == 0
    send_up(gpu, [frame_from(a, 99)])
    assert counters(gpu.acct_read([a])[0])[:2] == (99, 1)

    gpu.acct_add([b])                        # a live entry keeps its counters
    assert counters(gpu.acct_read([b])[0])[:2] == (141, 2)
    gpu.acct_add([b], reset=True)
    assert counters(gpu.acct_read([b])[0]) == (0,) * 7
    assert counters(gpu.acct_read([c])[0])[:2] == (161, 2)

    # 16 slots: the 17th distinct address finds no slot
    more = [ip2u32("198.18.0.1") + i for i in range(13)]
    gpu.acct_add(more)
    assert gpu.acct_count == 16
    with pytest.raises(RuntimeError, match="acct_log2"):
        gpu.acct_add([ip2u32("198.19.0.1")])
    assert gpu.acct_count == 16 and len(gpu.acct_export()) == 16
    with pytest.raises(ValueError):
        gpu.acct_add([a, a])                 # the batch contract


# --------------------------------------------------------------- off is off
def test_off_means_off():
    ip = ip2u32("192.0.2.1")
    never, was = plain_launcher(13), plain_launcher(13)
    assert never.acct is None and never.acct_count == 0
    assert len(never.acct_export()) == 0
    assert rows(never.acct_read([ip])) == [(0,) * 8]

    was.acct_add([ip])
    send_up(was, [frame_from(ip, 60)])
    assert was.acct_launches == {"resolve": 1, "commit": 1, "downlink": 0}
    assert counters(was.acct_remove([ip])[0])[:2] == (60, 1)
    assert was.acct_count == 0
    ran = dict(was.acct_launches)

    up = [mix_frame(i) for i in range(70)] + [frame_from(ip, 64)]
    down = [build_ipv4(CORE_MAC, SERVER_MAC, DST, ip, proto=17, sport=53,
                       dport=4000, payload=bytes(20 + i)) for i in range(5)]
    out = []
    for l in (never, was):
        d, ln = l.make_batch(up, stride=STRIDE)
        v, ol = l.uplink(d, ln, now_ns=NOW_NS, now_sec=NOW_SEC)
        d2, l2 = l.make_batch(down, stride=STRIDE)
        v2 = l.downlink(d2, l2, now_ns=NOW2_NS)
        out.append([t.cpu().numpy() for t in (v, ol, d, ln, v2, d2, l2)])
    for x, y in zip(*out):
        assert (x == y).all()
    assert never.acct is None
    assert never.acct_launches == {"resolve": 0, "commit": 0, "downlink": 0}
    assert was.acct_launches == ran          # nothing launched since
    assert len(was.acct_export()) == 0
