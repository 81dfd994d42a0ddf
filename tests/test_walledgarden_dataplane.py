"""The walled-garden gate off the device: the golden decision table
(GoldenDataplane.garden_uplink / garden_downlink — the source of truth the
gate kernels are differential-tested against), its agreement with
Manager.classify(), the GoldenLauncher wg_* surface, the golden Pump's
routing, the attach_dataplane glue and the `bng run` wiring."""
import ctypes
import itertools

import pytest

from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import DROP, FWD, PASS, GoldenDataplane
from bng_amd.dataplane.launcher import GoldenLauncher
from bng_amd.dataplane.packets import (DHCP_REQUEST, build_dhcp_request,
                                       ip2u32, u32_to_ip)
from bng_amd.walledgarden import manager as wgm
from bng_amd.walledgarden.dataplane import attach_dataplane
from wg_frames import (ALLOWED, CORE_MAC, DNS, OTHER, PORTAL, PORTAL_PORT,
                       SERVER_MAC, arp_from, raw_ipv4, vlan_tagged)

MAC_W = bytes.fromhex("aabbcc000001")        # quarantined
MAC_B = bytes.fromhex("aabbcc000002")        # blocked
MAC_X = bytes.fromhex("aabbcc0000ff")        # someone else's
IP_W = ip2u32("10.1.0.1")
IP_B = ip2u32("10.1.0.2")
IP_FREE = ip2u32("10.1.0.9")                 # not in the garden

NONE, ALLOW, REDIRECT = abi.WG_NONE, abi.WG_ALLOW, abi.WG_REDIRECT
D_WALLED, D_BLOCKED, D_MAC = (abi.WG_DROP_WALLED, abi.WG_DROP_BLOCKED,
                              abi.WG_DROP_MAC)


def garden():
    dp = GoldenDataplane()
    dp.wg_set_config(ALLOWED)
    dp.wg[IP_W] = (abi.mac_to_u64(MAC_W), abi.WG_WALLED)
    dp.wg[IP_B] = (abi.mac_to_u64(MAC_B), abi.WG_BLOCKED)
    return dp


def up(dst, proto, dport=0, *, src=IP_W, mac=MAC_W, **kw):
    return raw_ipv4(mac, SERVER_MAC, src, dst, proto, 40000, dport, **kw)


def down(src, proto, sport=0, *, dst=IP_W, **kw):
    return raw_ipv4(CORE_MAC, SERVER_MAC, src, dst, proto, sport, 40000, **kw)


def renewal(mac, ip):
    """A unicast DHCPREQUEST from the leased address."""
    f = build_dhcp_request(mac, DHCP_REQUEST, ciaddr=ip)
    return f[:26] + ip.to_bytes(4, "big") + f[30:]


# ------------------------------------------------------- the decision table
UPLINK_ROWS = [
    # row 1: not eligible, or source not in the table
    ("source not in the garden", up(OTHER, 6, 443, src=IP_FREE), NONE, None),
    ("ARP from a quarantined MAC", arp_from(MAC_W), NONE, None),
    ("VLAN-tagged data frame", vlan_tagged(up(OTHER, 6, 443)), NONE, None),
    ("version 5 under 08 00", up(OTHER, 6, 443, version=5), NONE, None),
    ("ihl 4", up(OTHER, 6, 443, ihl=5)[:14] + b"\x44" +
     up(OTHER, 6, 443)[15:], NONE, None),
    ("33 bytes", up(OTHER, 1)[:33], NONE, None),
    # row 2
    ("blocked", up(PORTAL, 6, PORTAL_PORT, src=IP_B, mac=MAC_B), D_BLOCKED,
     DROP),
    ("blocked, wrong MAC too", up(OTHER, 17, 53, src=IP_B, mac=MAC_X),
     D_BLOCKED, DROP),
    # row 3
    ("walled, another MAC", up(PORTAL, 6, PORTAL_PORT, mac=MAC_X), D_MAC,
     DROP),
    # row 4
    ("DHCP renewal", renewal(MAC_W, IP_W), NONE, None),
    ("UDP 67, plain", up(OTHER, 17, 67), NONE, None),
    ("TCP 67 is not DHCP", up(OTHER, 6, 67), D_WALLED, DROP),
    # row 5
    ("portal", up(PORTAL, 6, PORTAL_PORT), ALLOW, FWD),
    ("resolver over UDP", up(DNS, 17, 53), ALLOW, FWD),
    ("resolver over TCP", up(DNS, 6, 53), ALLOW, FWD),
    ("portal, ihl 6", up(PORTAL, 6, PORTAL_PORT, ihl=6), ALLOW, FWD),
    ("resolver, ihl 8: ports straddle 16-B words", up(DNS, 17, 53, ihl=8),
     ALLOW, FWD),
    ("resolver, ihl 15", up(DNS, 17, 53, ihl=15), ALLOW, FWD),
    # row 6
    ("HTTP", up(OTHER, 6, 80), REDIRECT, PASS),
    ("HTTP 8080", up(OTHER, 6, 8080), REDIRECT, PASS),
    ("HTTP, ihl 6", up(OTHER, 6, 80, ihl=6), REDIRECT, PASS),
    ("HTTP to the portal's address, not its port", up(PORTAL, 6, 80),
     REDIRECT, PASS),
    ("UDP 80 is not HTTP", up(OTHER, 17, 80), D_WALLED, DROP),
    # row 7: portless, allow-listed address
    ("ICMP to the portal", up(PORTAL, 1), ALLOW, FWD),
    ("GRE to the resolver", up(DNS, 47), ALLOW, FWD),
    ("non-first fragment to the portal", up(PORTAL, 6, 443, frag=100),
     ALLOW, FWD),
    ("TCP cut at 34 to the portal", up(PORTAL, 6, 443, l4_len=0), ALLOW, FWD),
    ("TCP cut at 41 to the portal", up(PORTAL, 6, 443, l4_len=7), ALLOW, FWD),
    ("TCP cut at 53 to the portal", up(PORTAL, 6, 443, l4_len=19), ALLOW,
     FWD),
    ("UDP cut short to the resolver", up(DNS, 17, 9, l4_len=7), ALLOW, FWD),
    # row 8
    ("HTTPS elsewhere", up(OTHER, 6, 443), D_WALLED, DROP),
    ("portal, wrong port", up(PORTAL, 6, 443), D_WALLED, DROP),
    ("portal port over UDP", up(PORTAL, 17, PORTAL_PORT), D_WALLED, DROP),
    ("ICMP elsewhere", up(OTHER, 1), D_WALLED, DROP),
    ("non-first fragment elsewhere", up(OTHER, 6, 80, frag=100), D_WALLED,
     DROP),
    ("more-fragments on a first fragment keeps its ports",
     up(OTHER, 6, 80, frag=0x2000), REDIRECT, PASS),
    ("TCP cut at 53 elsewhere: no port, no redirect",
     up(OTHER, 6, 80, l4_len=19), D_WALLED, DROP),
    ("HTTP, ihl 6, cut inside the TCP header", up(OTHER, 6, 80, ihl=6,
                                                   l4_len=19), D_WALLED, DROP),
]


@pytest.mark.parametrize("row", UPLINK_ROWS, ids=[r[0] for r in UPLINK_ROWS])
def test_uplink_table(row):
    _name, frame, gate, verdict = row
    dp = garden()
    before = bytes(frame)
    assert dp.garden_uplink(frame) == (gate, verdict)
    assert bytes(frame) == before
    want = [0] * abi.WG_NSTATS
    if gate != NONE:
        want[{ALLOW: abi.WS_UP_ALLOWED, REDIRECT: abi.WS_UP_REDIRECTED,
              D_WALLED: abi.WS_UP_DROP_WALLED,
              D_BLOCKED: abi.WS_UP_DROP_BLOCKED,
              D_MAC: abi.WS_UP_DROP_MAC}[gate]] = 1
    assert dp.wg_stats == want


def test_truncated_lengths_are_the_ones_the_issue_names():
    assert [len(up(PORTAL, 6, 443, l4_len=k)) for k in (0, 7, 19)] == \
        [34, 41, 53]
    assert len(up(PORTAL, 6, 443)) == 54
    f = up(PORTAL, 6, PORTAL_PORT, ihl=6)
    assert f[14] == 0x46 and f[38:42] == (40000).to_bytes(2, "big") + \
        PORTAL_PORT.to_bytes(2, "big")


DOWNLINK_ROWS = [
    ("to nobody in the garden", down(OTHER, 17, 53, dst=IP_FREE), FWD, NONE,
     FWD),
    ("not forwarded: untouched", down(DNS, 17, 53), DROP, NONE, DROP),
    ("passed: untouched", down(OTHER, 6, 80), PASS, NONE, PASS),
    ("blocked", down(DNS, 17, 53, dst=IP_B), FWD, D_BLOCKED, DROP),
    ("from the resolver", down(DNS, 17, 53), FWD, ALLOW, FWD),
    ("from the portal", down(PORTAL, 6, PORTAL_PORT), FWD, ALLOW, FWD),
    ("from the portal, ihl 7", down(PORTAL, 6, PORTAL_PORT, ihl=7), FWD,
     ALLOW, FWD),
    ("from the portal's other port", down(PORTAL, 6, 443), FWD, D_WALLED,
     DROP),
    ("from elsewhere", down(OTHER, 6, 80), FWD, D_WALLED, DROP),
    ("ICMP from the portal", down(PORTAL, 1), FWD, ALLOW, FWD),
    ("ICMP from elsewhere", down(OTHER, 1), FWD, D_WALLED, DROP),
    ("fragment from the resolver", down(DNS, 17, 53, frag=9), FWD, ALLOW,
     FWD),
    ("fragment from elsewhere", down(OTHER, 17, 53, frag=9), FWD, D_WALLED,
     DROP),
    ("tagged", vlan_tagged(down(OTHER, 6, 80)), FWD, NONE, FWD),
]


@pytest.mark.parametrize("row", DOWNLINK_ROWS,
                         ids=[r[0] for r in DOWNLINK_ROWS])
def test_downlink_table(row):
    _name, frame, verdict, gate, out = row
    dp = garden()
    assert dp.garden_downlink(frame, verdict) == (gate, out)
    assert sum(dp.wg_stats[:abi.WS_DOWN_ALLOWED]) == 0
    assert sum(dp.wg_stats) == (0 if gate == NONE else 1)


# ------------------------------------------------ agreement with the manager
def test_gate_agrees_with_manager_classify():
    """Rows 5-8 against Manager.classify on the full grid; a frame without
    readable ports (ICMP, or port 0 built as a non-first fragment) is
    classified with port 0."""
    dests = {"portal": PORTAL, "dns": DNS, "other": OTHER}
    ports = [0, 53, 80, 443, 8080, PORTAL_PORT]
    macs = {"walled": MAC_W, "blocked": MAC_B,
            "active": bytes.fromhex("aabbcc000003"),
            "unknown": bytes.fromhex("aabbcc000004")}
    ips = {"walled": IP_W, "blocked": IP_B, "active": ip2u32("10.1.0.3"),
           "unknown": ip2u32("10.1.0.4")}
    mstr = {k: ":".join(f"{b:02x}" for b in v) for k, v in macs.items()}
    m = wgm.Manager(portal_ip=u32_to_ip(PORTAL), dns_servers=[u32_to_ip(DNS)],
                    portal_port=PORTAL_PORT)
    l = GoldenLauncher()
    attach_dataplane(m, l)
    for st in ("walled", "blocked", "active"):
        m.add(mstr[st], u32_to_ip(ips[st]))
    m.block(mstr["blocked"])
    m.activate(mstr["active"])
    assert l.wg_count == 2
    want = {wgm.V_FORWARD: {NONE, ALLOW}, wgm.V_REDIRECT: {REDIRECT},
            wgm.V_DROP: {D_WALLED, D_BLOCKED}}
    seen = set()
    for (dn, dst), port, proto, st in itertools.product(
            dests.items(), ports, (6, 17, 1), macs):
        readable = proto != 1 and port != 0
        frame = raw_ipv4(macs[st], SERVER_MAC, ips[st], dst, proto, 40000,
                         port, frag=0 if readable or proto == 1 else 64)
        gate, verdict = l.dp.garden_uplink(frame)
        cls = m.classify(mstr[st], u32_to_ip(dst), port if readable else 0,
                         proto)
        assert gate in want[cls], (dn, port, proto, st, gate, cls)
        assert verdict == {NONE: None, ALLOW: FWD, REDIRECT: PASS}.get(
            gate, DROP)
        seen.add(gate)
    assert seen == {NONE, ALLOW, REDIRECT, D_WALLED, D_BLOCKED}


# ---------------------------------------------------------- allow-list edges
def keys(n):
    return [(ip2u32("10.9.0.0") + 7 * i, 1000 + i, 6) for i in range(n)]


@pytest.mark.parametrize("n", [0, 1, 64])
def test_allow_list_sizes(n):
    dp = GoldenDataplane()
    dp.wg_set_config(keys(n))
    dp.wg[IP_W] = (abi.mac_to_u64(MAC_W), abi.WG_WALLED)
    for i in ([0, n - 1] if n else []):               # first and last key
        ip, port, proto = keys(n)[i]
        assert dp.garden_uplink(up(ip, proto, port))[0] == ALLOW
        assert dp.garden_uplink(up(ip, proto, port + 1))[0] == D_WALLED
        assert dp.garden_uplink(up(ip, 1))[0] == ALLOW       # bare address
    assert dp.garden_uplink(up(ip2u32("10.8.0.1"), 6, 1000))[0] == D_WALLED
    assert dp.garden_uplink(up(ip2u32("10.8.0.1"), 1))[0] == D_WALLED


def test_keys_that_differ_in_one_field_only():
    dp = GoldenDataplane()
    dp.wg_set_config([(DNS, 53, 17), (DNS, 54, 6), (DNS, 53, 17)])  # folds
    dp.wg[IP_W] = (abi.mac_to_u64(MAC_W), abi.WG_WALLED)
    assert len(dp.wg_allowed) == 2 and dp.wg_allowed_ips == {DNS}
    assert dp.garden_uplink(up(DNS, 17, 53))[0] == ALLOW
    assert dp.garden_uplink(up(DNS, 6, 53))[0] == D_WALLED    # proto only
    assert dp.garden_uplink(up(DNS, 6, 54))[0] == ALLOW
    assert dp.garden_uplink(up(DNS, 17, 54))[0] == D_WALLED   # proto only
    assert dp.garden_uplink(up(DNS, 17, 52))[0] == D_WALLED   # port only


@pytest.mark.parametrize("make", [GoldenDataplane, GoldenLauncher])
def test_config_capacity(make):
    g = make()
    g.wg_set_config(keys(64), redirect_ports=range(1, 9))
    with pytest.raises(ValueError, match="64"):
        g.wg_set_config(keys(65))
    with pytest.raises(ValueError, match="8"):
        g.wg_set_config(keys(1), redirect_ports=range(1, 10))


def test_redirect_ports_come_from_the_config():
    dp = garden()
    dp.wg_set_config(ALLOWED, redirect_ports=(8000,))
    assert dp.garden_uplink(up(OTHER, 6, 8000)) == (REDIRECT, PASS)
    assert dp.garden_uplink(up(OTHER, 6, 80)) == (D_WALLED, DROP)


# ------------------------------------------------- GoldenLauncher surface
def test_golden_launcher_surface():
    l = GoldenLauncher(wg_log2=4)
    assert l.wg_count == 0 and len(l.wg_export()) == 0
    assert l.wg_get_stats() == dict.fromkeys(abi.WG_STAT_NAMES, 0)
    l.wg_set_config(ALLOWED)
    l.wg_set([(IP_W, MAC_W, abi.WG_WALLED), (IP_B, MAC_B, abi.WG_BLOCKED)])
    with pytest.raises(ValueError, match="repeat"):
        l.wg_set([(IP_FREE, MAC_X, abi.WG_WALLED),
                  (IP_FREE, MAC_W, abi.WG_WALLED)])
    with pytest.raises(ValueError, match="state"):
        l.wg_set([(IP_FREE, MAC_X, 0)])
    assert l.wg_count == 2
    assert l.dp.garden_uplink(up(PORTAL, 6, PORTAL_PORT))[0] == ALLOW
    l.wg_set([(IP_W, MAC_W, abi.WG_BLOCKED)])         # in place
    assert l.wg_count == 2
    assert l.dp.garden_uplink(up(PORTAL, 6, PORTAL_PORT))[0] == D_BLOCKED
    l.wg_set([(IP_W, abi.mac_to_u64(MAC_X), abi.WG_WALLED)])   # MAC as int
    assert l.dp.garden_uplink(up(PORTAL, 6, PORTAL_PORT))[0] == D_MAC
    exp = l.wg_export()
    assert len(exp) == l.wg_count == 2
    assert sorted(int(k) for k in exp["key"]) == sorted(
        abi.wg_key(ip) for ip in (IP_W, IP_B))
    row = exp[exp["key"] == abi.wg_key(IP_W)][0]
    assert int(row["mac_state"]) == abi.wg_mac_state(
        abi.mac_to_u64(MAC_X), abi.WG_WALLED)
    l.wg_remove([IP_W, IP_FREE])                      # absent: ignored
    assert l.wg_count == 1
    assert l.dp.garden_uplink(up(PORTAL, 6, PORTAL_PORT))[0] == NONE
    st = l.wg_get_stats()
    assert list(st) == abi.WG_STAT_NAMES
    assert (st["up_allowed"], st["up_drop_blocked"], st["up_drop_mac"]) == \
        (1, 1, 1)


# --------------------------------------------------------------- Pump routing
def test_pump_routes_by_gate_both_directions():
    from bng_amd.dataplane.pktio import Pump
    l = GoldenLauncher()
    l.wg_set_config(ALLOWED)
    frames = [up(PORTAL, 6, PORTAL_PORT), up(OTHER, 6, 80),
              up(OTHER, 6, 443), up(OTHER, 17, 53, src=IP_B, mac=MAC_B),
              up(ip2u32("198.51.100.7"), 17, 53, src=ip2u32("192.0.2.9"))]
    # empty garden: the quarantined source is a private address without a
    # port block, which the NAT stage passes to the host
    p0 = Pump(l, None)
    out0, passed0 = p0.process(frames)
    assert p0.stats["passed"] == 4 and p0.stats["fwd"] == 1
    assert l.wg_get_stats() == dict.fromkeys(abi.WG_STAT_NAMES, 0)

    l.wg_set([(IP_W, MAC_W, abi.WG_WALLED), (IP_B, MAC_B, abi.WG_BLOCKED)])
    p = Pump(l, None)
    out, passed = p.process(frames)
    assert out == [frames[0], frames[4]]              # ALLOW: untouched
    assert passed == [frames[1]]                      # REDIRECT: to the host
    assert (p.stats["fwd"], p.stats["passed"], p.stats["dropped"]) == \
        (2, 1, 2)
    st = l.wg_get_stats()
    assert (st["up_allowed"], st["up_redirected"], st["up_drop_walled"],
            st["up_drop_blocked"]) == (1, 1, 1, 1)

    back = [down(DNS, 17, 53), down(OTHER, 6, 80),
            down(DNS, 17, 53, dst=IP_B), down(OTHER, 17, 53, dst=IP_FREE)]
    d = Pump(l, None, direction="downlink")
    out, passed = d.process(back)
    assert out == [back[0], back[3]] and passed == []
    assert (d.stats["fwd"], d.stats["dropped"]) == (2, 2)
    st = l.wg_get_stats()
    assert (st["down_allowed"], st["down_drop_walled"],
            st["down_drop_blocked"]) == (1, 1, 1)


def test_pump_accounts_allowed_and_dropped():
    from bng_amd.dataplane.pktio import Pump
    l = GoldenLauncher()
    l.wg_set_config(ALLOWED)
    l.wg_set([(IP_W, MAC_W, abi.WG_WALLED)])
    l.acct_add([IP_W])
    f = up(PORTAL, 6, PORTAL_PORT)
    Pump(l, None).process([f, up(OTHER, 6, 443), up(OTHER, 6, 80)])
    e = l.acct_read([IP_W])[0]
    assert (int(e["up_pkts"]), int(e["up_bytes"]), int(e["up_drop_pkts"])) \
        == (1, len(f), 1)


# ------------------------------------------------- attach_dataplane lifecycle
class Recorder(GoldenLauncher):
    def __init__(self):
        super().__init__()
        self.calls = []

    def wg_set_config(self, allowed, redirect_ports=(80, 8080)):
        self.calls.append(("config", sorted(allowed), tuple(redirect_ports)))
        super().wg_set_config(allowed, redirect_ports)

    def wg_set(self, entries):
        entries = list(entries)
        self.calls.append(("set", entries))
        super().wg_set(entries)

    def wg_remove(self, ips):
        ips = list(ips)
        self.calls.append(("remove", ips))
        super().wg_remove(ips)


def test_attach_dataplane_lifecycle():
    m = wgm.Manager(portal_ip=u32_to_ip(PORTAL), dns_servers=[u32_to_ip(DNS)],
                    portal_port=PORTAL_PORT)
    m.add("AA:BB:CC:00:00:07", "10.1.0.7")            # present before attach
    m.add("aa:bb:cc:00:00:08", "")                    # no address: skipped
    l = Recorder()
    attach_dataplane(m, l)
    assert l.calls[0] == ("config", sorted(ALLOWED), (80, 8080))
    assert l.dp.wg == {ip2u32("10.1.0.7"):
                       (0xAABBCC000007, abi.WG_WALLED)}

    mac = "aa:bb:cc:00:00:01"
    m.add(mac, u32_to_ip(IP_W))
    assert l.dp.wg[IP_W] == (abi.mac_to_u64(MAC_W), abi.WG_WALLED)
    m.block(mac)
    assert l.dp.wg[IP_W] == (abi.mac_to_u64(MAC_W), abi.WG_BLOCKED)
    assert not m.activate(mac)                        # blocked stays blocked
    assert IP_W in l.dp.wg
    m.remove(mac)                                     # notifies a stale state
    assert IP_W not in l.dp.wg

    m.add(mac, u32_to_ip(IP_W))
    assert m.activate(mac)
    assert IP_W not in l.dp.wg and l.calls[-1] == ("remove", [IP_W])
    m.remove(mac)

    m.add(mac, u32_to_ip(IP_W), ttl=5)
    m.add(mac, "10.1.0.44", ttl=5)                    # same MAC, new lease
    assert IP_W not in l.dp.wg and ip2u32("10.1.0.44") in l.dp.wg
    assert m.expire_stale(now=m.entries[mac].added_at + 6) == 1
    assert ip2u32("10.1.0.44") not in l.dp.wg
    assert l.wg_count == 1                            # the adopted entry

    n_cfg = sum(1 for c in l.calls if c[0] == "config")
    m.allow_destination("192.0.2.80", 443, 6)
    assert sum(1 for c in l.calls if c[0] == "config") == n_cfg + 1
    assert (ip2u32("192.0.2.80"), 443, 6) in l.dp.wg_allowed
    assert ip2u32("192.0.2.80") in l.dp.wg_allowed_ips
    assert len(l.dp.wg_allowed) == len(ALLOWED) + 1


def test_allow_destination_callbacks_are_optional():
    m = wgm.Manager(portal_ip="10.0.0.1")
    m.allow_destination("192.0.2.1", 443, 6)          # nobody listens
    hits = []
    m.on_destinations_changed(lambda: hits.append(1))
    m.on_destinations_changed(lambda: 1 / 0)          # a bad listener
    m.allow_destination("192.0.2.2", 443, 6)
    assert hits == [1] and m.is_destination_allowed("192.0.2.2", 443, 6)


# ------------------------------------------------------------------- layouts
def test_ctypes_layouts():
    assert ctypes.sizeof(abi.WgEntry) == 16
    assert ctypes.sizeof(abi.WgConfig) == 800
    assert abi.EXPECTED_SIZES["bng_wg_entry"] == (abi.WgEntry, 16)
    assert abi.EXPECTED_SIZES["bng_wg_config"] == (abi.WgConfig, 800)
    assert abi.WgEntry.mac_state.offset == 8
    assert (abi.WgConfig.allowed_key.offset, abi.WgConfig.allowed_ip.offset,
            abi.WgConfig.redirect_port.offset) == (16, 528, 784)
    assert (abi.MAX_WG_LOG2, abi.MAX_WG_ALLOWED,
            abi.MAX_WG_REDIRECT_PORTS) == (21, 64, 8)
    assert (abi.WG_WALLED, abi.WG_BLOCKED) == (1, 2)
    assert [abi.WG_NONE, abi.WG_ALLOW, abi.WG_REDIRECT, abi.WG_DROP_WALLED,
            abi.WG_DROP_BLOCKED, abi.WG_DROP_MAC] == list(range(6))
    assert abi.WG_STAT_NAMES == [
        "up_allowed", "up_redirected", "up_drop_walled", "up_drop_blocked",
        "up_drop_mac", "down_allowed", "down_drop_walled",
        "down_drop_blocked"]
    assert len(abi.WG_STAT_NAMES) == abi.WG_NSTATS == 8
    assert abi.wg_key(0) == 1 << 32 != abi.KEY_EMPTY
    assert abi.wg_key(0xFFFFFFFF) == 0x1FFFFFFFF != abi.KEY_TOMBSTONE
    assert abi.wg_key(IP_W) == abi.acct_key(IP_W)
    assert abi.wg_mac_state(0xAABBCC000001, 2) == 0x0200AABBCC000001
    assert abi.wg_allowed_key(0x0A000001, 53, 17) == 0x0A00000100350011


def test_extension_reports_the_wg_layout():
    from bng_amd.dataplane.build import get_ext
    ext = get_ext()
    if ext is None:
        pytest.skip("extension not built")
    rep = ext.layout_report()
    assert rep["bng_wg_entry"] == 16 and rep["bng_wg_config"] == 800
    assert rep["offsets"]["wg_entry.mac_state"] == 8
    for f in ("allowed_key", "allowed_ip", "redirect_port"):
        assert rep["offsets"][f"wg_config.{f}"] == \
            getattr(abi.WgConfig, f).offset


# ------------------------------------------------------------- bng run wiring
def test_bng_run_wires_the_garden_to_the_dataplane():
    from bng_amd.cli.main import BNG, build_parser
    args = build_parser().parse_args([
        "run", "--pool-network", "10.0.1.0/24", "--pool-gateway", "10.0.1.1",
        "--gpu", "off", "--walled-garden"])
    app = BNG(args).start()
    try:
        portal = ip2u32("10.255.255.1")
        assert (portal, 8080, 6) in app.launcher.dp.wg_allowed
        mac = "aa:bb:cc:00:00:01"
        app.walledgarden.add(mac, "10.0.1.77")
        ip = ip2u32("10.0.1.77")
        assert app.launcher.dp.wg[ip] == (abi.mac_to_u64(MAC_W),
                                          abi.WG_WALLED)
        redirects = []
        app.walledgarden.on_redirect(lambda m, d: redirects.append((m, d)))
        http = up(OTHER, 6, 80, src=ip)
        assert app.launcher.dp.garden_uplink(http) == (REDIRECT, PASS)
        assert app._frame_slow_path(http) is None
        assert redirects == [(mac, u32_to_ip(OTHER))]
        assert app.walledgarden.stats["redirects"] == 1
        # not a quarantined MAC, not TCP: no redirect is counted
        assert not app._garden_redirect(up(OTHER, 6, 80, src=ip, mac=MAC_X))
        assert not app._garden_redirect(up(OTHER, 17, 80, src=ip))
        assert len(redirects) == 1
        st = app.stats()
        assert st["walledgarden_gate"]["up_redirected"] == 1
        assert st["walledgarden"]["redirects"] == 1
        app.walledgarden.activate(mac)
        assert ip not in app.launcher.dp.wg
    finally:
        app.stop()


def test_metrics_export_the_gate_counters():
    from bng_amd.metrics.metrics import Metrics
    l = GoldenLauncher()
    l.wg_set_config(ALLOWED)
    l.wg_set([(IP_W, MAC_W, abi.WG_WALLED)])
    l.dp.garden_uplink(up(OTHER, 6, 443))
    m = Metrics()
    m.collect_once(l)
    get = m.registry.get_sample_value
    assert get("bng_dataplane_stat",
               {"module": "walledgarden", "name": "up_drop_walled"}) == 1
    assert get("bng_dataplane_stat",
               {"module": "walledgarden", "name": "up_allowed"}) == 0
