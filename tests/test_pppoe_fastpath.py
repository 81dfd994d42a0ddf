"""PPPoE session-data fast path — golden model, ABI, pump and CLI wiring.

The golden model is the oracle for the two device kernels
(tests/test_pppoe_fastpath_gpu.py), so its rules are pinned here one by
one: every REJECT reason, CTRL for the PPP control protocols, padding
trimmed on decap, the TOO_BIG / NO_ROOM boundaries on encap, and each of
the eight counters.
"""
import ctypes
import struct

import pytest

from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import DROP, FWD, PASS, GoldenDataplane
from bng_amd.dataplane.launcher import GoldenLauncher
from bng_amd.dataplane.packets import build_ipv4, ip2u32
from bng_amd.dataplane.pktio import Pump
from bng_amd.pppoe import codec as C

NOW_NS = 1_700_000_000 * 10**9
SERVER_MAC = bytes.fromhex("020000000001")
CORE_MAC = bytes.fromhex("020000000002")
MAC_A = bytes.fromhex("aabbcc000011")
MAC_B = bytes.fromhex("aabbcc000022")
IP_A = ip2u32("10.1.0.11")
IP_B = ip2u32("10.1.0.22")
DST = ip2u32("93.184.216.34")
SID_A, SID_B = 0x0102, 0xFFFF


def ipoe(mac=MAC_A, src=IP_A, payload=b"", sport=4000):
    return build_ipv4(mac, SERVER_MAC, src, DST, proto=17, sport=sport,
                      dport=53, payload=payload)


def wrap(frame, sid=SID_A, proto=C.PROTO_IPV4):
    """The PPPoE session frame carrying an IPoE frame's IP packet."""
    return C.SessionPacket(sid, proto, frame[14:], src_mac=frame[6:12],
                           dst_mac=frame[0:6]).encode()


def pattern(n):
    return bytes((7 * i + 3) & 0xFF for i in range(n))


def stats(dp):
    return dict(zip(abi.PPPOE_STAT_NAMES, dp.pppoe_stats))


@pytest.fixture
def dp():
    d = GoldenDataplane(now_ns=NOW_NS)
    d.server_mac = SERVER_MAC
    d.pppoe_add_session(SID_A, MAC_A, IP_A, 1492)
    d.pppoe_add_session(SID_B, MAC_B, IP_B, 100)
    return d


# ------------------------------------------------------------------ decap
class TestGoldenDecap:
    def test_data_frame_becomes_its_ipoe_twin(self, dp):
        twin = ipoe(payload=pattern(37))
        fb = bytearray(wrap(twin))
        st, n = dp.pppoe_decap(fb)
        assert (st, n) == (abi.PPPOE_DECAP, len(twin))
        assert bytes(fb[:n]) == twin
        assert stats(dp)["decap_ok"] == 1
        assert sum(dp.pppoe_stats) == 1

    def test_bare_header_is_the_smallest_decap(self, dp):
        twin = ipoe()[:34]                       # 20-byte IP "packet"
        fb = bytearray(wrap(twin))
        assert dp.pppoe_decap(fb) == (abi.PPPOE_DECAP, 34)
        assert bytes(fb[:34]) == twin

    def test_ethernet_padding_is_trimmed(self, dp):
        twin = ipoe()[:34]
        fb = bytearray(wrap(twin).ljust(60, b"\x00"))
        assert len(fb) == 60
        assert dp.pppoe_decap(fb) == (abi.PPPOE_DECAP, 34)
        assert bytes(fb[:34]) == twin

    @pytest.mark.parametrize("et", [0x0800, 0x8863, 0x0806, 0x8100, 0x86DD])
    def test_other_ethertypes_untouched(self, dp, et):
        f = SERVER_MAC + MAC_A + struct.pack(">H", et) + pattern(40)
        fb = bytearray(f)
        assert dp.pppoe_decap(fb) == (abi.PPPOE_NONE, len(f))
        assert bytes(fb) == f
        assert sum(dp.pppoe_stats) == 0

    def test_vlan_tagged_pppoe_is_out_of_scope(self, dp):
        inner = wrap(ipoe())
        f = inner[:12] + b"\x81\x00\x00\x64" + inner[12:]
        fb = bytearray(f)
        assert dp.pppoe_decap(fb) == (abi.PPPOE_NONE, len(f))
        assert bytes(fb) == f

    def test_short_frames(self, dp):
        assert dp.pppoe_decap(bytearray(b"\x00" * 10)) == (abi.PPPOE_NONE, 10)
        f = bytearray(wrap(ipoe())[:21])
        assert dp.pppoe_decap(f) == (abi.PPPOE_REJECT, 21)
        assert stats(dp)["decap_malformed"] == 1

    @pytest.mark.parametrize("off,val", [(14, 0x21), (15, 0x01)])
    def test_bad_version_or_code(self, dp, off, val):
        good = wrap(ipoe())
        fb = bytearray(good)
        fb[off] = val
        want = bytes(fb)
        assert dp.pppoe_decap(fb) == (abi.PPPOE_REJECT, len(good))
        assert bytes(fb) == want
        assert stats(dp)["decap_malformed"] == 1
        assert sum(dp.pppoe_stats) == 1

    @pytest.mark.parametrize("plen", [0, 1])
    def test_payload_length_below_two(self, dp, plen):
        fb = bytearray(wrap(ipoe()))
        struct.pack_into(">H", fb, 18, plen)
        assert dp.pppoe_decap(fb)[0] == abi.PPPOE_REJECT
        assert stats(dp)["decap_malformed"] == 1

    def test_payload_length_past_the_frame(self, dp):
        good = wrap(ipoe())
        fb = bytearray(good)
        struct.pack_into(">H", fb, 18, len(good) - 20 + 1)
        assert dp.pppoe_decap(fb)[0] == abi.PPPOE_REJECT
        assert stats(dp)["decap_malformed"] == 1
        fb = bytearray(good)                     # exactly to the end: fine
        assert dp.pppoe_decap(fb)[0] == abi.PPPOE_DECAP

    @pytest.mark.parametrize("proto", [C.PROTO_LCP, C.PROTO_IPCP,
                                       C.PROTO_IPV6, C.PROTO_CHAP,
                                       C.PROTO_IPV6CP])
    def test_control_protocols_are_ctrl_even_without_a_session(self, dp,
                                                               proto):
        f = C.SessionPacket(0x0777, proto, pattern(12), src_mac=MAC_B,
                            dst_mac=SERVER_MAC).encode()
        fb = bytearray(f)
        assert dp.pppoe_decap(fb) == (abi.PPPOE_CTRL, len(f))
        assert bytes(fb) == f
        assert stats(dp)["decap_ctrl"] == 1
        assert sum(dp.pppoe_stats) == 1

    def test_unknown_session(self, dp):
        good = wrap(ipoe(), sid=0x0103)
        fb = bytearray(good)
        assert dp.pppoe_decap(fb) == (abi.PPPOE_REJECT, len(good))
        assert bytes(fb) == good
        assert stats(dp)["decap_unknown_session"] == 1
        assert sum(dp.pppoe_stats) == 1

    def test_mac_mismatch(self, dp):
        good = wrap(ipoe(mac=MAC_B))             # B's MAC on A's session
        fb = bytearray(good)
        assert dp.pppoe_decap(fb) == (abi.PPPOE_REJECT, len(good))
        assert bytes(fb) == good
        assert stats(dp)["decap_mac_mismatch"] == 1
        assert sum(dp.pppoe_stats) == 1

    def test_ip_packet_shorter_than_a_header(self, dp):
        f = C.SessionPacket(SID_A, C.PROTO_IPV4, pattern(19), src_mac=MAC_A,
                            dst_mac=SERVER_MAC).encode()
        assert dp.pppoe_decap(bytearray(f))[0] == abi.PPPOE_REJECT
        assert stats(dp)["decap_malformed"] == 1
        f = C.SessionPacket(SID_A, C.PROTO_IPV4, pattern(20), src_mac=MAC_A,
                            dst_mac=SERVER_MAC).encode()
        assert dp.pppoe_decap(bytearray(f))[0] == abi.PPPOE_DECAP

    def test_rule_order_ctrl_before_session_lookup_before_mac(self, dp):
        # LCP on an unknown session with a foreign MAC is still CTRL
        f = C.SessionPacket(0x0999, C.PROTO_LCP, b"\x01\x01\x00\x04",
                            src_mac=MAC_B, dst_mac=SERVER_MAC).encode()
        assert dp.pppoe_decap(bytearray(f))[0] == abi.PPPOE_CTRL
        # unknown session wins over the short-IP check
        f = C.SessionPacket(0x0999, C.PROTO_IPV4, pattern(4), src_mac=MAC_A,
                            dst_mac=SERVER_MAC).encode()
        assert dp.pppoe_decap(bytearray(f))[0] == abi.PPPOE_REJECT
        assert stats(dp)["decap_unknown_session"] == 1


# ------------------------------------------------------------------ encap
def reply(dst_ip, payload=b"", n=None):
    f = build_ipv4(CORE_MAC, SERVER_MAC, DST, dst_ip, proto=17, sport=53,
                   dport=4000, payload=payload)
    return f if n is None else f.ljust(n, b"\x5a")[:n]


class TestGoldenEncap:
    def test_encap_fields(self, dp):
        f = reply(IP_A, pattern(33))
        fb = bytearray(f)
        st, v, n = dp.pppoe_encap(fb, FWD, 512)
        assert (st, v, n) == (abi.PPPOE_ENCAP, FWD, len(f) + 8)
        p = C.SessionPacket.decode(bytes(fb[:n]))
        assert p.session_id == SID_A and p.ppp_proto == C.PROTO_IPV4
        assert p.dst_mac == MAC_A and p.src_mac == SERVER_MAC
        assert p.payload == f[14:]
        assert fb[14] == 0x11 and fb[15] == 0x00
        assert struct.unpack_from(">H", fb, 18)[0] == len(f) - 14 + 2
        assert stats(dp) == dict(zip(abi.PPPOE_STAT_NAMES,
                                     [0, 0, 0, 0, 0, 1, 0, 0]))

    def test_encap_then_decap_is_identity_on_the_ip_packet(self, dp):
        for k in (0, 1, 4, 7, 8, 9, 15, 16, 300):
            f = reply(IP_A, pattern(k))
            fb = bytearray(f)
            st, v, n = dp.pppoe_encap(fb, FWD, 512)
            assert st == abi.PPPOE_ENCAP
            # the client answers from its own MAC
            back = bytearray(fb[:n])
            back[0:6], back[6:12] = SERVER_MAC, MAC_A
            st, m = dp.pppoe_decap(back)
            assert st == abi.PPPOE_DECAP and m == len(f)
            assert bytes(back[14:m]) == f[14:]

    @pytest.mark.parametrize("verdict", [PASS, DROP, abi.TX])
    def test_only_forwarded_frames(self, dp, verdict):
        f = reply(IP_A)
        fb = bytearray(f)
        assert dp.pppoe_encap(fb, verdict, 512) == (abi.PPPOE_NONE, verdict,
                                                    len(f))
        assert bytes(fb) == f and sum(dp.pppoe_stats) == 0

    def test_non_ipv4_short_and_miss_untouched(self, dp):
        arp = SERVER_MAC + CORE_MAC + b"\x08\x06" + pattern(46)
        short = reply(IP_A)[:33]
        miss = reply(ip2u32("10.1.0.99"))
        for f in (arp, short, miss):
            fb = bytearray(f)
            assert dp.pppoe_encap(fb, FWD, 512) == (abi.PPPOE_NONE, FWD,
                                                    len(f))
            assert bytes(fb) == f
        assert sum(dp.pppoe_stats) == 0

    def test_too_big_boundary(self, dp):
        # session B has MRU 100
        ok = reply(IP_B, n=14 + 100)
        fb = bytearray(ok)
        assert dp.pppoe_encap(fb, FWD, 512)[0] == abi.PPPOE_ENCAP
        big = reply(IP_B, n=14 + 101)
        fb = bytearray(big)
        assert dp.pppoe_encap(fb, FWD, 512) == (abi.PPPOE_TOO_BIG, PASS,
                                                len(big))
        assert bytes(fb) == big
        st = stats(dp)
        assert st["encap_ok"] == 1 and st["encap_too_big"] == 1
        assert st["encap_no_room"] == 0

    @pytest.mark.parametrize("stride", [512, 2048])
    def test_no_room_boundary(self, stride):
        d = GoldenDataplane(now_ns=NOW_NS)
        d.server_mac = SERVER_MAC
        d.pppoe_add_session(SID_A, MAC_A, IP_A, 4000)
        ok = reply(IP_A, n=stride - 8)
        fb = bytearray(ok)
        st, v, n = d.pppoe_encap(fb, FWD, stride)
        assert (st, v, n) == (abi.PPPOE_ENCAP, FWD, stride)
        tight = reply(IP_A, n=stride - 7)
        fb = bytearray(tight)
        assert d.pppoe_encap(fb, FWD, stride) == (abi.PPPOE_NO_ROOM, PASS,
                                                  len(tight))
        assert bytes(fb) == tight
        st = stats(d)
        assert st["encap_ok"] == 1 and st["encap_no_room"] == 1

    def test_too_big_is_checked_before_no_room(self, dp):
        f = reply(IP_B, n=510)
        assert dp.pppoe_encap(bytearray(f), FWD, 512)[0] == abi.PPPOE_TOO_BIG


# -------------------------------------------------------------- lifecycle
class TestGoldenTables:
    def test_remove(self, dp):
        dp.pppoe_remove_session(SID_A)
        assert SID_A not in dp.pppoe_sessions and IP_A not in dp.pppoe_by_ip
        assert dp.pppoe_decap(bytearray(wrap(ipoe())))[0] == abi.PPPOE_REJECT
        assert dp.pppoe_encap(bytearray(reply(IP_A)), FWD, 512)[0] == \
            abi.PPPOE_NONE
        dp.pppoe_remove_session(SID_A)           # idempotent

    def test_reprovision_same_id_drops_the_stale_ip(self, dp):
        new_ip = ip2u32("10.1.0.33")
        dp.pppoe_add_session(SID_A, MAC_B, new_ip, 1400)
        assert IP_A not in dp.pppoe_by_ip
        assert dp.pppoe_by_ip[new_ip][0] == SID_A
        assert dp.pppoe_decap(bytearray(wrap(ipoe())))[0] == abi.PPPOE_REJECT
        assert stats(dp)["decap_mac_mismatch"] == 1
        assert dp.pppoe_encap(bytearray(reply(IP_A)), FWD, 512)[0] == \
            abi.PPPOE_NONE
        assert dp.pppoe_encap(bytearray(reply(new_ip)), FWD, 512)[0] == \
            abi.PPPOE_ENCAP

    def test_address_taken_over_by_a_newer_session(self, dp):
        dp.pppoe_add_session(0x0200, MAC_B, IP_A, 1492)
        assert dp.pppoe_by_ip[IP_A][0] == 0x0200
        dp.pppoe_remove_session(SID_A)           # must not evict the owner
        assert dp.pppoe_by_ip[IP_A][0] == 0x0200

    def test_launcher_surface(self):
        l = GoldenLauncher()
        l.set_server_config(SERVER_MAC, ip2u32("10.255.255.1"))
        assert l.pppoe_get_stats() == dict.fromkeys(abi.PPPOE_STAT_NAMES, 0)
        l.add_pppoe_session(SID_A, MAC_A, IP_A)
        assert l.dp.pppoe_sessions[SID_A].mru == 1492
        twin = ipoe(payload=pattern(5))
        data, lens = [bytearray(wrap(twin)), bytearray(twin)], [0, 0]
        lens[:] = [len(d) for d in data]
        assert l.pppoe_decap(data, lens) == [abi.PPPOE_DECAP, abi.PPPOE_NONE]
        assert lens == [len(twin), len(twin)]
        assert bytes(data[0][:lens[0]]) == twin
        back = [bytearray(reply(IP_A)), bytearray(reply(IP_B))]
        blens = [len(b) for b in back]
        verdict = [FWD, FWD]
        assert l.pppoe_encap(back, blens, verdict) == \
            [abi.PPPOE_ENCAP, abi.PPPOE_NONE]
        assert blens[0] == len(reply(IP_A)) + 8 and verdict == [FWD, FWD]
        st = l.pppoe_get_stats()
        assert st["decap_ok"] == 1 and st["encap_ok"] == 1
        l.remove_pppoe_session(SID_A)
        assert not l.dp.pppoe_sessions


# -------------------------------------------------------------------- ABI
def test_ctypes_sizes_and_fields():
    assert ctypes.sizeof(abi.PppoeSess) == 16
    assert ctypes.sizeof(abi.PppoeIp) == 16
    assert abi.EXPECTED_SIZES["bng_pppoe_sess"] == (abi.PppoeSess, 16)
    assert abi.EXPECTED_SIZES["bng_pppoe_ip"] == (abi.PppoeIp, 16)
    assert abi.PppoeSess.ip.offset == 8 and abi.PppoeSess.mru.offset == 12
    assert abi.PppoeIp.sid_mac.offset == 8
    assert len(abi.PPPOE_STAT_NAMES) == abi.PPPOE_NSTATS == 8
    assert (abi.PPPOE_NONE, abi.PPPOE_DECAP, abi.PPPOE_CTRL,
            abi.PPPOE_REJECT, abi.PPPOE_ENCAP, abi.PPPOE_TOO_BIG,
            abi.PPPOE_NO_ROOM) == (0, 1, 2, 3, 4, 5, 6)
    assert abi.pppoe_ip_key(0) not in (abi.KEY_EMPTY, abi.KEY_TOMBSTONE)
    assert abi.pppoe_ip_key(0xFFFFFFFF) == 0x1FFFFFFFF


def test_extension_layout_report_has_the_pppoe_structs():
    from bng_amd.dataplane.build import get_ext
    ext = get_ext()
    if ext is None:
        pytest.skip("extension not built")
    rep = ext.layout_report()
    assert rep["bng_pppoe_sess"] == 16 and rep["bng_pppoe_ip"] == 16
    off = rep["offsets"]
    assert off["pppoe_sess.ip"] == abi.PppoeSess.ip.offset
    assert off["pppoe_sess.mru"] == abi.PppoeSess.mru.offset
    assert off["pppoe_sess.session_id"] == abi.PppoeSess.session_id.offset
    assert off["pppoe_ip.sid_mac"] == abi.PppoeIp.sid_mac.offset


# ------------------------------------------------------------------- pump
def provisioned_launcher():
    l = GoldenLauncher()
    l.dp.now_ns = NOW_NS
    l.set_server_config(SERVER_MAC, ip2u32("10.255.255.1"))
    l.set_antispoof_config(default_mode=abi.AS_STRICT)
    l.add_binding(MAC_A, ipv4=IP_A, mode=abi.AS_STRICT)
    l.add_subscriber_nat(IP_A, ip2u32("203.0.113.1"), 1024, 1535,
                         subscriber_id=1)
    l.add_pppoe_session(SID_A, MAC_A, IP_A)
    return l


class TestPump:
    def test_data_frame_equals_its_ipoe_twin_and_skips_the_slow_path(self):
        twin = ipoe(payload=pattern(21))
        seen = []
        a = Pump(provisioned_launcher(), None, slow_path=seen.append)
        b = Pump(provisioned_launcher(), None, slow_path=seen.append)
        out_a, passed_a = a.process([twin])
        out_b, passed_b = b.process([wrap(twin)])
        assert len(out_a) == 1 and out_a == out_b
        assert out_a[0] != twin                  # it really was NAT-ed
        assert struct.unpack_from(">I", out_a[0], 26)[0] == \
            ip2u32("203.0.113.1")
        assert passed_a == passed_b == [] and seen == []
        assert a.stats == b.stats and b.stats["fwd"] == 1
        assert b.launcher.pppoe_get_stats()["decap_ok"] == 1

    def test_lcp_still_reaches_the_slow_path(self):
        lcp = C.SessionPacket(SID_A, C.PROTO_LCP, C.CPPacket(
            C.ECHO_REQ, 1, b"\x00" * 4).encode(), src_mac=MAC_A,
            dst_mac=SERVER_MAC).encode()
        seen = []
        p = Pump(provisioned_launcher(), None,
                 slow_path=lambda f: seen.append(f))
        out, passed = p.process([lcp])
        assert passed == [lcp] and seen == [lcp] and out == []
        assert p.stats["passed"] == 1 and p.stats["dropped"] == 0
        assert p.launcher.pppoe_get_stats()["decap_ctrl"] == 1

    def test_unknown_session_data_is_dropped(self):
        bad = wrap(ipoe(), sid=0x0BAD)
        seen = []
        p = Pump(provisioned_launcher(), None, slow_path=seen.append)
        out, passed = p.process([bad])
        assert out == [] and passed == [] and seen == []
        assert p.stats["dropped"] == 1 and p.stats["passed"] == 0
        assert p.launcher.pppoe_get_stats()["decap_unknown_session"] == 1

    def test_no_sessions_keeps_todays_routing(self):
        l = provisioned_launcher()
        l.remove_pppoe_session(SID_A)
        f = wrap(ipoe())
        p = Pump(l, None)
        out, passed = p.process([f])
        assert passed == [f] and out == []
        assert sum(l.dp.pppoe_stats) == 0

    def test_round_trip_both_ways(self):
        """Uplink PPPoE data is NAT-ed out; the reply comes back wrapped in
        the subscriber's session."""
        l = provisioned_launcher()
        up = Pump(l, None)
        down = Pump(l, None, direction="downlink")
        twin = ipoe(payload=pattern(9))
        out, _ = up.process([wrap(twin)])
        nat_ip = struct.unpack_from(">I", out[0], 26)[0]
        nat_port = struct.unpack_from(">H", out[0], 34)[0]
        back = build_ipv4(CORE_MAC, SERVER_MAC, DST, nat_ip, proto=17,
                          sport=53, dport=nat_port, payload=pattern(13))
        other = build_ipv4(CORE_MAC, SERVER_MAC, DST, ip2u32("198.51.100.7"),
                           proto=17, sport=53, dport=9, payload=b"x")
        got, passed = down.process([back, other])
        assert passed == [] and len(got) == 2
        p = C.SessionPacket.decode(got[0])
        assert p.session_id == SID_A and p.ppp_proto == C.PROTO_IPV4
        assert p.dst_mac == MAC_A and p.src_mac == SERVER_MAC
        assert struct.unpack_from(">I", p.payload, 16)[0] == IP_A
        assert struct.unpack_from(">H", p.payload, 22)[0] == 4000
        assert p.payload[28:] == pattern(13)
        assert got[1] == other                   # not a PPPoE subscriber

    def test_downlink_too_big_goes_to_passed(self):
        l = provisioned_launcher()
        l.add_pppoe_session(SID_A, MAC_A, IP_A, mru=60)
        down = Pump(l, None, direction="downlink")
        f = build_ipv4(CORE_MAC, SERVER_MAC, DST, IP_A, proto=17, sport=53,
                       dport=9, payload=pattern(64))
        got, passed = down.process([f])
        assert got == [] and passed == [f]
        assert down.stats["passed"] == 1
        assert l.pppoe_get_stats()["encap_too_big"] == 1


# -------------------------------------------------------------------- CLI
def test_cli_hooks_provision_and_remove_the_fast_path_session():
    """`bng run --pppoe-enable`: IPCP-open adds the session to the
    launcher, teardown removes it, and in between the golden Pump moves an
    IP packet both ways."""
    from bng_amd.cli.main import BNG, build_parser
    from tests.test_pppoe import SimClient
    argv = ["run", "--pool-network", "10.0.1.0/24", "--pool-gateway",
            "10.0.1.1", "--pool-dns", "8.8.8.8", "--gpu", "off",
            "--pppoe-enable", "--pppoe-auth", "none", "--nat-enable",
            "--nat-public-ip", "203.0.113.1", "--qos-policy", "gold:100:20",
            "--qos-default-policy", "gold", "--metrics-enable",
            "--metrics-port", "0"]
    app = BNG(build_parser().parse_args(argv)).start()
    try:
        app.pppoe.local_users = {}
        cli = SimClient(app.pppoe, username="u1")
        cli.discover()
        sess = list(app.pppoe.sessions.values())[0]
        rec = app.launcher.dp.pppoe_sessions[sess.session_id]
        assert rec.ip == sess.ip and rec.mru == sess.peer_mru
        assert rec.mac == abi.mac_to_u64(sess.client_mac)
        assert app.launcher.dp.pppoe_by_ip[sess.ip][0] == sess.session_id

        server_mac = app.launcher.dp.server_mac
        twin = build_ipv4(sess.client_mac, server_mac, sess.ip, DST,
                          proto=17, sport=4000, dport=53,
                          payload=pattern(11))
        up = Pump(app.launcher, None, slow_path=app._frame_slow_path)
        out, passed = up.process([wrap(twin, sid=sess.session_id)])
        assert passed == [] and len(out) == 1
        assert out[0][12:14] == b"\x08\x00"
        nat_ip = struct.unpack_from(">I", out[0], 26)[0]
        nat_port = struct.unpack_from(">H", out[0], 34)[0]
        assert nat_ip == ip2u32("203.0.113.1")
        down = Pump(app.launcher, None, direction="downlink")
        back = build_ipv4(CORE_MAC, server_mac, DST, nat_ip, proto=17,
                          sport=53, dport=nat_port, payload=pattern(5))
        got, _ = down.process([back])
        p = C.SessionPacket.decode(got[0])
        assert p.session_id == sess.session_id
        assert p.dst_mac == sess.client_mac
        assert struct.unpack_from(">I", p.payload, 16)[0] == sess.ip

        app.metrics.collect_once(app.launcher, app.dhcp_server)
        text = app.metrics.render().decode()
        assert "bng_pppoe_fastpath_decap_ok_total 1.0" in text
        assert "bng_pppoe_fastpath_encap_ok_total 1.0" in text
        for name in abi.PPPOE_STAT_NAMES:
            assert f"bng_pppoe_fastpath_{name}_total" in text

        app.pppoe.terminate_session(sess.session_id)
        assert sess.session_id not in app.launcher.dp.pppoe_sessions
        assert sess.ip not in app.launcher.dp.pppoe_by_ip
    finally:
        app.stop()
