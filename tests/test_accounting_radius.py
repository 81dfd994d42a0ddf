"""Dataplane counters to RADIUS, end to end on the CPU: a DHCP server over
a GoldenLauncher, TrafficAccounting, and an AccountingManager against the
in-process RADIUS server — plus the accounting request's wire encoding
(Gigawords, packet counts) and the persisted-state compatibility."""
import json
import struct

import pytest

from bng_amd.accounting.traffic import TrafficAccounting
from bng_amd.dataplane import abi
from bng_amd.dataplane.launcher import GoldenLauncher
from bng_amd.dataplane.packets import build_ipv4, ip2u32, mac_bytes, u32_to_ip
from bng_amd.dataplane.pktio import Pump
from bng_amd.dhcp import message as dm
from bng_amd.dhcp.pool import PoolConfig, PoolManager
from bng_amd.dhcp.server import DHCPServer
from bng_amd.radius import packet as rp
from bng_amd.radius.accounting import AccountingManager, SessionRecord
from bng_amd.radius.client import Client
from bng_amd.radius.server import RadiusServer

SECRET = b"s3cr3t"
MAC = mac_bytes("aa:bb:cc:00:00:01")
SERVER_MAC = bytes.fromhex("020000000001")
CORE_MAC = bytes.fromhex("020000000002")
DST = ip2u32("93.184.216.34")
PUBLIC = ip2u32("203.0.113.1")


@pytest.fixture
def server():
    srv = RadiusServer(SECRET, users={}).start()
    yield srv
    srv.stop()


def records(server, status):
    return [r for r in server.acct_records
            if r.get_int(rp.ACCT_STATUS_TYPE) == status]


def octets(rec, lo, hi):
    """The 64-bit count a record's Octets + Gigawords pair carries."""
    return rec.get_int(lo) + ((rec.get_int(hi) or 0) << 32)


# ------------------------------------------------------------- end to end
def test_interim_and_stop_carry_the_dataplane_counters(server):
    launcher = GoldenLauncher()
    pm = PoolManager(launcher)
    pm.add_pool(PoolConfig(1, "10.0.1.0/24", gateway="10.0.1.1",
                           dns=["8.8.8.8"], lease_time=600))
    dhcp = DHCPServer(pm, "10.0.0.1")
    dhcp.set_launcher(launcher)
    am = AccountingManager(Client([server.addr], SECRET),
                           interim_interval=9999)
    dhcp.set_accounting(am)
    ta = TrafficAccounting(launcher)
    dhcp.on_lease_event.append(ta.on_lease_event)
    am.set_counter_fetcher(ta.fetch)

    offer = dhcp.handle(dm.build_request(MAC, dm.DISCOVER))
    ip = offer.yiaddr
    assert launcher.acct_count == 0          # an offer is not a session
    ack = dhcp.handle(dm.build_request(MAC, dm.REQUEST, requested_ip=ip))
    assert ack.msg_type == dm.ACK
    assert launcher.acct_count == 1
    assert int(launcher.acct_read([ip])[0]["key"]) == abi.acct_key(ip)
    assert len(records(server, rp.ACCT_START)) == 1
    (sid,) = am.sessions

    launcher.add_subscriber_nat(ip, PUBLIC, 1024, 1535, subscriber_id=1)
    up = [build_ipv4(MAC, SERVER_MAC, ip, DST, proto=17, sport=4000,
                     dport=53, payload=bytes(n)) for n in (18, 58, 30)]
    out, _ = Pump(launcher, None).process(up)
    assert len(out) == 3
    nat_port = struct.unpack_from(">H", out[0], 34)[0]
    down = [build_ipv4(CORE_MAC, SERVER_MAC, DST, PUBLIC, proto=17, sport=53,
                       dport=nat_port, payload=bytes(n)) for n in (100, 7)]
    got, _ = Pump(launcher, None, direction="downlink").process(down)
    assert len(got) == 2
    e = launcher.dp.acct[ip]
    assert (e.up_bytes, e.up_pkts) == (sum(map(len, up)), 3)
    assert (e.down_bytes, e.down_pkts) == (sum(map(len, down)), 2)

    # a renewal keeps the entry and its counters
    dhcp.handle(dm.build_request(MAC, dm.REQUEST, requested_ip=ip))
    assert launcher.dp.acct[ip].up_pkts == 3

    assert am.send_interim(sid)
    (interim,) = records(server, rp.ACCT_INTERIM)
    assert interim.get_int(rp.ACCT_INPUT_OCTETS) == e.up_bytes
    assert interim.get_int(rp.ACCT_OUTPUT_OCTETS) == e.down_bytes
    assert interim.get_int(rp.ACCT_INPUT_PACKETS) == 3
    assert interim.get_int(rp.ACCT_OUTPUT_PACKETS) == 2
    assert interim.get(rp.ACCT_INPUT_GIGAWORDS) is None
    assert launcher.acct_count == 1          # an interim removes nothing

    # more traffic, then the lease goes: the device entry is gone before
    # the Stop record is built, and the record still has the final counts
    Pump(launcher, None).process(up[:1])
    dhcp.handle(dm.build_request(MAC, dm.RELEASE, ciaddr=ip))
    assert launcher.acct_count == 0 and ip not in launcher.dp.acct
    (stop,) = records(server, rp.ACCT_STOP)
    assert stop.get_str(rp.ACCT_SESSION_ID) == sid
    assert stop.get_int(rp.ACCT_INPUT_OCTETS) == \
        sum(map(len, up)) + len(up[0])
    assert stop.get_int(rp.ACCT_INPUT_PACKETS) == 4
    assert stop.get_int(rp.ACCT_OUTPUT_OCTETS) == sum(map(len, down))
    assert stop.get_int(rp.ACCT_OUTPUT_PACKETS) == 2
    assert ta._final == {}                   # the parked final was used up
    assert am.sessions == {}


def test_fetch_prefers_a_parked_final_and_knows_absent_addresses():
    launcher = GoldenLauncher()
    ta = TrafficAccounting(launcher)
    ip = ip2u32("10.0.1.9")
    lease = type("Lease", (), {"ip": ip})()
    rec = SessionRecord("s1", "alice", framed_ip=u32_to_ip(ip))
    assert ta.fetch(rec) is None             # nobody accounts it yet
    assert ta.fetch(SessionRecord("s2", "bob")) is None      # no address
    ta.on_lease_event("add", lease)
    launcher.dp.acct_commit(ip, "uplink", 1000, abi.FWD, 5)
    launcher.dp.acct_commit(ip, "downlink", 3000, abi.FWD, 6)
    assert ta.fetch(rec) == (1000, 3000, 1, 1)               # a live read
    ta.on_lease_event("delete", lease)
    assert launcher.acct_count == 0
    # the address is re-leased before the old Stop record is built: the old
    # session still gets its own final counts, once
    launcher.acct_add([ip])
    assert ta.fetch(rec) == (1000, 3000, 1, 1)
    assert ta.fetch(rec) == (0, 0, 0, 0)                     # the new entry
    ta.on_lease_event("delete", lease)
    ta.on_lease_event("delete", lease)       # twice: nothing to park
    ta.on_lease_event("add", lease)          # a new owner drops a stale final
    assert ta._final == {}


def test_two_tuple_fetcher_still_works(server):
    am = AccountingManager(Client([server.addr], SECRET),
                           interim_interval=9999)
    am.set_counter_fetcher(lambda rec: (11, 22))
    sid = am.start_session("alice", framed_ip="10.0.1.50")
    am.stop_session(sid)
    (stop,) = records(server, rp.ACCT_STOP)
    assert stop.get_int(rp.ACCT_INPUT_OCTETS) == 11
    assert stop.get_int(rp.ACCT_OUTPUT_OCTETS) == 22
    assert stop.get(rp.ACCT_INPUT_PACKETS) is None


# ---------------------------------------------------------- wire encoding
def test_gigawords_above_32_bits_only(server):
    c = Client([server.addr], SECRET)
    big = 5 * 2**32 + 7
    assert c.send_accounting(rp.ACCT_STOP, "s", "alice", "10.0.1.50",
                             big, 2**32 - 1, 60, 1)
    r = server.acct_records[-1]
    assert r.get_int(rp.ACCT_INPUT_OCTETS) == 7
    assert r.get_int(rp.ACCT_INPUT_GIGAWORDS) == 5
    assert octets(r, rp.ACCT_INPUT_OCTETS, rp.ACCT_INPUT_GIGAWORDS) == big
    # exactly 0xFFFFFFFF still fits: no Gigawords attribute
    assert r.get_int(rp.ACCT_OUTPUT_OCTETS) == 2**32 - 1
    assert r.get(rp.ACCT_OUTPUT_GIGAWORDS) is None
    assert c.send_accounting(rp.ACCT_INTERIM, "s", "alice", "10.0.1.50",
                             100, 2**32, 60)
    r = server.acct_records[-1]
    assert r.get(rp.ACCT_INPUT_GIGAWORDS) is None
    assert r.get_int(rp.ACCT_OUTPUT_OCTETS) == 0
    assert r.get_int(rp.ACCT_OUTPUT_GIGAWORDS) == 1
    assert (rp.ACCT_INPUT_GIGAWORDS, rp.ACCT_OUTPUT_GIGAWORDS) == (52, 53)


def test_packet_counts_only_when_given(server):
    c = Client([server.addr], SECRET)
    assert c.send_accounting(rp.ACCT_INTERIM, "s", "alice", "10.0.1.50",
                             100, 200, 60, input_packets=3,
                             output_packets=2**32 + 4)
    r = server.acct_records[-1]
    assert r.get_int(rp.ACCT_INPUT_PACKETS) == 3
    assert r.get_int(rp.ACCT_OUTPUT_PACKETS) == 4
    assert c.send_accounting(rp.ACCT_INTERIM, "s", "alice", "10.0.1.50",
                             100, 200, 60, input_packets=0)
    r = server.acct_records[-1]
    assert r.get_int(rp.ACCT_INPUT_PACKETS) == 0     # given, even if zero
    assert r.get(rp.ACCT_OUTPUT_PACKETS) is None


def legacy_request(nas_id, status, session_id, username, framed_ip,
                   input_octets, output_octets, session_time,
                   terminate_cause, mac):
    """The attribute list send_accounting built before it knew Gigawords
    and packet counts."""
    import socket
    pkt = rp.Packet(rp.ACCOUNTING_REQUEST, 0)
    pkt.add(rp.ACCT_STATUS_TYPE, status)
    pkt.add(rp.ACCT_SESSION_ID, session_id)
    if username:
        pkt.add(rp.USER_NAME, username)
    if framed_ip:
        pkt.add(rp.FRAMED_IP_ADDRESS, struct.pack(">I", int.from_bytes(
            socket.inet_aton(framed_ip), "big")))
    if mac:
        pkt.add(rp.CALLING_STATION_ID, mac)
    pkt.add(rp.NAS_IDENTIFIER, nas_id)
    if status in (rp.ACCT_INTERIM, rp.ACCT_STOP):
        pkt.add(rp.ACCT_INPUT_OCTETS, input_octets & 0xFFFFFFFF)
        pkt.add(rp.ACCT_OUTPUT_OCTETS, output_octets & 0xFFFFFFFF)
        pkt.add(rp.ACCT_SESSION_TIME, session_time)
    if status == rp.ACCT_STOP and terminate_cause:
        pkt.add(rp.ACCT_TERMINATE_CAUSE, terminate_cause)
    return pkt.attributes


@pytest.mark.parametrize("args", [
    (rp.ACCT_START, "s-1", "alice", "10.0.1.50", 0, 0, 0, 0, ""),
    (rp.ACCT_INTERIM, "s-1", "alice", "10.0.1.50", 1000, 2000, 60, 0,
     "aa:bb:cc:00:00:01"),
    (rp.ACCT_STOP, "s-1", "alice", "10.0.1.50", 2**32 - 1, 0, 90, 1,
     "aa:bb:cc:00:00:01"),
    (rp.ACCT_STOP, "s-2", "", "", 5, 6, 7, 0, ""),
], ids=["start", "interim", "stop", "bare-stop"])
def test_requests_of_todays_callers_are_unchanged(server, args):
    c = Client([server.addr], SECRET)
    assert c.send_accounting(*args)
    got = server.acct_records[-1].attributes
    want = legacy_request(c.nas_identifier, *args)
    assert len(got) == len(want)
    for g, w in zip(got, want):              # attribute by attribute
        assert g == w


def test_manager_without_packet_fetcher_sends_the_old_request(server):
    am = AccountingManager(Client([server.addr], SECRET),
                           interim_interval=9999)
    sid = am.start_session("alice", mac="aa:bb:cc:00:00:01",
                           framed_ip="10.0.1.50")
    am.update_counters(sid, 1000, 2000)
    am.stop_session(sid)
    (stop,) = records(server, rp.ACCT_STOP)
    types = [t for t, _ in stop.attributes]
    assert rp.ACCT_INPUT_PACKETS not in types
    assert rp.ACCT_INPUT_GIGAWORDS not in types
    assert stop.get_int(rp.ACCT_INPUT_OCTETS) == 1000


# ------------------------------------------------------------- persistence
def test_old_persisted_state_still_recovers_its_orphans(server, tmp_path):
    path = tmp_path / "acct.json"
    old = {"session_id": "orphan-1", "username": "alice", "mac": "",
           "framed_ip": "10.0.1.50", "start_time": 1_700_000_000.0,
           "input_octets": 123, "output_octets": 456, "last_interim": 0.0,
           "stopped": False, "terminate_cause": 0}
    assert "input_packets" not in old
    path.write_text(json.dumps({"sessions": {"orphan-1": old},
                                "pending": []}))
    am = AccountingManager(Client([server.addr], SECRET),
                           persist_path=str(path), interim_interval=9999)
    (item,) = am.pending
    assert item["status"] == rp.ACCT_STOP and item["orphan"]
    assert item["rec"]["input_packets"] == 0
    assert am.flush_pending() == 1
    stop = server.acct_records[-1]
    assert stop.get_str(rp.ACCT_SESSION_ID) == "orphan-1"
    assert stop.get_int(rp.ACCT_INPUT_OCTETS) == 123
    assert stop.get(rp.ACCT_INPUT_PACKETS) is None
