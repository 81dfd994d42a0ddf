"""Per-subscriber traffic accounting, CPU side: the golden model's rules
(the device kernels are differential-tested against them in
test_accounting_gpu.py), GoldenLauncher's table semantics, the pump's
golden branches and the ABI mirror."""
import ctypes
import struct

import numpy as np
import pytest

from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import (DROP, FWD, PASS, TX, AcctRec,
                                      GoldenDataplane)
from bng_amd.dataplane.launcher import GoldenLauncher
from bng_amd.dataplane.packets import build_ipv4, ip2u32
from bng_amd.dataplane.pktio import Pump

NOW_NS = 1_700_000_000 * 10**9
SUB = ip2u32("10.1.0.7")
OTHER = ip2u32("198.51.100.8")       # a public address: NAT leaves it alone
PUBLIC = ip2u32("203.0.113.1")
DST = ip2u32("93.184.216.34")
SUB_MAC = bytes.fromhex("aabbcc000007")
SERVER_MAC = bytes.fromhex("020000000001")
CORE_MAC = bytes.fromhex("020000000002")


def up_frame(src=SUB, length=64, sport=4000):
    f = build_ipv4(SUB_MAC, SERVER_MAC, src, DST, proto=17, sport=sport,
                   dport=53, payload=bytes(length - 42))
    assert len(f) == length
    return f


def down_frame(dst=SUB, length=64, dport=4000):
    return build_ipv4(CORE_MAC, SERVER_MAC, DST, dst, proto=17, sport=53,
                      dport=dport, payload=bytes(length - 42))


def tagged(f):
    return f[:12] + b"\x81\x00\x00\x64" + f[12:]


def counters(e):
    return tuple(getattr(e, f) for f in abi.ACCT_COUNTERS)


# ------------------------------------------------------------ golden rules
# direction, verdict -> (up_bytes, up_pkts, down_bytes, down_pkts,
#                        up_drop_pkts, down_drop_pkts, last_seen)
COMMIT_RULES = [
    ("uplink", FWD, (90, 1, 0, 0, 0, 0, NOW_NS)),
    ("uplink", DROP, (0, 0, 0, 0, 1, 0, 0)),
    ("uplink", PASS, (0,) * 7),
    ("uplink", TX, (0,) * 7),
    ("downlink", FWD, (0, 0, 90, 1, 0, 0, NOW_NS)),
    ("downlink", DROP, (0, 0, 0, 0, 0, 1, 0)),
    ("downlink", PASS, (0,) * 7),
    ("downlink", TX, (0,) * 7),
]


@pytest.mark.parametrize("direction,verdict,want", COMMIT_RULES)
def test_commit_rule(direction, verdict, want):
    l = GoldenLauncher()
    l.acct_add([SUB])
    l.dp.acct_commit(SUB, direction, 90, verdict, NOW_NS)
    assert counters(l.dp.acct[SUB]) == want


RESOLVE_RULES = [
    ("src", up_frame(), SUB),
    ("dst", up_frame(), None),                   # DST is nobody's
    ("dst", down_frame(), SUB),
    ("src", down_frame(), None),
    ("src", up_frame(src=OTHER), None),          # an absent key
    ("src", tagged(up_frame()), None),           # tagged: not the data path
    ("dst", tagged(down_frame()), None),
    ("src", up_frame()[:33], None),              # too short to hold dst
    ("src", up_frame()[:34], SUB),
    ("src", up_frame()[:12] + b"\x86\xdd" + up_frame()[14:], None),   # IPv6
    ("src", SERVER_MAC + SUB_MAC + b"\x08\x06" + bytes(28), None),    # ARP
    ("src", b"", None),
]


@pytest.mark.parametrize("by,frame,want", RESOLVE_RULES)
def test_resolve_rule(by, frame, want):
    dp = GoldenDataplane(now_ns=NOW_NS)
    dp.acct[SUB] = AcctRec()
    assert dp.acct_resolve(frame, by) == want
    assert dp.acct_resolve(bytearray(frame), by) == want


def test_commit_to_nobody_is_a_no_op():
    dp = GoldenDataplane()
    dp.acct_commit(None, "uplink", 90, FWD, NOW_NS)
    dp.acct_commit(SUB, "uplink", 90, FWD, NOW_NS)     # not accounted
    assert dp.acct == {}


def nat_launcher():
    l = GoldenLauncher()
    l.dp.now_ns = NOW_NS
    l.set_server_config(SERVER_MAC, ip2u32("10.255.255.1"))
    l.add_subscriber_nat(SUB, PUBLIC, 1024, 1535, subscriber_id=1)
    l.acct_add([SUB])
    return l


def test_uplink_is_keyed_before_nat_and_downlink_after():
    l = nat_launcher()
    dp = l.dp
    fb = bytearray(up_frame(length=77))
    key = dp.acct_resolve(fb, "src")
    assert dp.nat44_egress(fb) == FWD
    assert struct.unpack_from(">I", fb, 26)[0] == PUBLIC      # rewritten
    assert dp.acct_resolve(fb, "src") is None      # too late to key it now
    dp.acct_commit(key, "uplink", len(fb), FWD, NOW_NS)
    nat_port = struct.unpack_from(">H", fb, 34)[0]

    back = bytearray(down_frame(dst=PUBLIC, length=99, dport=nat_port))
    assert dp.acct_resolve(back, "dst") is None    # still the public address
    assert dp.nat44_ingress(back) == FWD
    assert dp.acct_resolve(back, "dst") == SUB
    dp.acct_commit(SUB, "downlink", len(back), FWD, NOW_NS + 5)
    assert counters(dp.acct[SUB]) == (77, 1, 99, 1, 0, 0, NOW_NS + 5)


# ------------------------------------------------- GoldenLauncher semantics
def test_launcher_add_read_remove_export():
    l = GoldenLauncher(acct_log2=4)
    assert l.acct_count == 0 and len(l.acct_export()) == 0
    l.acct_add([SUB, OTHER])
    assert l.acct_count == 2
    l.dp.acct_commit(SUB, "uplink", 100, FWD, NOW_NS)
    l.dp.acct_commit(SUB, "downlink", 60, DROP, NOW_NS)
    r = l.acct_read([OTHER, SUB, DST])
    assert r.dtype == np.dtype(abi.ACCT_ENTRY_DTYPE)
    assert [int(k) for k in r["key"]] == [abi.acct_key(OTHER),
                                         abi.acct_key(SUB), 0]
    assert tuple(int(x) for x in r[1]) == (
        abi.acct_key(SUB), 100, 1, 0, 0, 0, 1, NOW_NS)
    assert tuple(int(x) for x in r[2]) == (0,) * 8     # absent: a zero row

    l.acct_add([SUB])                        # a live entry keeps its counters
    assert int(l.acct_read([SUB])[0]["up_bytes"]) == 100
    l.acct_add([SUB], reset=True)
    assert tuple(int(x) for x in l.acct_read([SUB])[0])[1:] == (0,) * 7

    l.dp.acct_commit(SUB, "uplink", 40, FWD, NOW_NS)
    exp = l.acct_export()
    assert sorted(int(k) for k in exp["key"]) == sorted(
        [abi.acct_key(SUB), abi.acct_key(OTHER)])
    final = l.acct_remove([SUB, DST])
    assert tuple(int(x) for x in final[0]) == (
        abi.acct_key(SUB), 40, 1, 0, 0, 0, 0, NOW_NS)
    assert int(final[1]["key"]) == 0
    assert l.acct_count == 1 and int(l.acct_read([SUB])[0]["key"]) == 0
    l.acct_add([SUB])                        # a new entry starts from zero
    assert tuple(int(x) for x in l.acct_read([SUB])[0])[1:] == (0,) * 7
    with pytest.raises(ValueError):
        l.acct_add([SUB, SUB])


# --------------------------------------------------------------------- pump
def test_pump_over_golden_updates_entries_both_ways():
    l = nat_launcher()
    l.set_qos_policy(OTHER, 8000, 10, direction="ingress", now_ns=NOW_NS)
    l.acct_add([OTHER])
    up = Pump(l, None)
    out, passed = up.process([
        up_frame(length=70), up_frame(length=81, sport=4001),
        up_frame(src=OTHER, length=64),              # QoS: always drops
        up_frame(src=ip2u32("10.1.0.9"), length=64),   # nobody accounts it
        tagged(up_frame()),
        SERVER_MAC + SUB_MAC + b"\x08\x06" + bytes(28),
    ])
    # no port block: the host's; and the ARP frame
    assert up.stats["dropped"] == 1 and len(passed) == 2
    assert counters(l.dp.acct[SUB]) == (151, 2, 0, 0, 0, 0, NOW_NS)
    assert counters(l.dp.acct[OTHER]) == (0, 0, 0, 0, 1, 0, 0)

    snat = [f for f in out
            if struct.unpack_from(">I", f, 26)[0] == PUBLIC]
    assert len(snat) == 2
    nat_port = struct.unpack_from(">H", snat[0], 34)[0]
    down = Pump(l, None, direction="downlink")
    got, _ = down.process([
        down_frame(dst=PUBLIC, length=120, dport=nat_port),
        down_frame(dst=ip2u32("10.1.0.9"), length=64),
    ])
    assert len(got) >= 1
    assert struct.unpack_from(">I", got[0], 30)[0] == SUB
    assert counters(l.dp.acct[SUB]) == (151, 2, 120, 1, 0, 0, NOW_NS)


def test_pump_counts_the_ipoe_length_of_pppoe_frames():
    from bng_amd.pppoe import codec as C
    l = nat_launcher()
    l.add_pppoe_session(0x0011, SUB_MAC, SUB)
    twin = up_frame(length=77)
    wire = C.SessionPacket(0x0011, C.PROTO_IPV4, twin[14:], src_mac=SUB_MAC,
                           dst_mac=SERVER_MAC).encode()
    bad = bytearray(wire)
    bad[6:12] = bytes.fromhex("aabbcc0000ff")          # wrong MAC: rejected
    up = Pump(l, None)
    out, _ = up.process([wire, bytes(bad)])
    assert len(out) == 1 and up.stats["dropped"] == 1
    assert counters(l.dp.acct[SUB])[:2] == (len(wire) - 8, 1)
    assert l.dp.acct[SUB].up_drop_pkts == 0

    nat_port = struct.unpack_from(">H", out[0], 34)[0]
    back = down_frame(dst=PUBLIC, length=90, dport=nat_port)
    got, _ = Pump(l, None, direction="downlink").process([back])
    assert len(got) == 1 and len(got[0]) == len(back) + 8
    assert counters(l.dp.acct[SUB])[2:4] == (len(back), 1)


# ---------------------------------------------------------------------- ABI
def test_acct_entry_dtype_matches_ctypes():
    dt = np.dtype(abi.ACCT_ENTRY_DTYPE)
    assert dt.itemsize == 64 == ctypes.sizeof(abi.AcctEntry)
    assert list(dt.names) == [f[0] for f in abi.AcctEntry._fields_]
    for name, ctype in abi.AcctEntry._fields_:
        assert dt.fields[name][1] == getattr(abi.AcctEntry, name).offset, name
        assert dt.fields[name][0].itemsize == ctypes.sizeof(ctype), name
    assert abi.ACCT_COUNTERS == list(dt.names)[1:]
    assert abi.EXPECTED_SIZES["bng_acct_entry"] == (abi.AcctEntry, 64)
    assert abi.MAX_ACCT_LOG2 == 21


def test_acct_key_is_never_empty_or_tombstone():
    assert abi.acct_key(0) == 1 << 32 != abi.KEY_EMPTY
    assert abi.acct_key(0xFFFFFFFF) == 0x1FFFFFFFF != abi.KEY_TOMBSTONE
    assert abi.acct_key(SUB) & 0xFFFFFFFF == SUB
    assert abi.acct_key(SUB + (1 << 32)) == abi.acct_key(SUB)


def test_extension_reports_the_acct_layout():
    from bng_amd.dataplane.build import get_ext
    ext = get_ext()
    if ext is None:
        pytest.skip("extension not built")
    rep = ext.layout_report()
    assert rep["bng_acct_entry"] == 64
    for f in ("up_bytes", "down_bytes", "up_drop_pkts", "last_seen"):
        assert rep["offsets"][f"acct_entry.{f}"] == \
            getattr(abi.AcctEntry, f).offset


# ------------------------------------------------------------------ metrics
def test_metrics_collector_sets_session_bytes_from_entries():
    from bng_amd.metrics.metrics import Metrics
    l = nat_launcher()
    m = Metrics()
    m.collect_once(l)
    l.dp.acct_commit(SUB, "uplink", 500, FWD, NOW_NS)
    l.dp.acct_commit(SUB, "downlink", 900, FWD, NOW_NS)
    m.collect_once(l)
    m.collect_once(l)                        # a second pull adds nothing
    get = m.registry.get_sample_value
    assert get("bng_session_bytes_in_total", {"access_type": "dhcp"}) == 500
    assert get("bng_session_bytes_out_total", {"access_type": "dhcp"}) == 900
