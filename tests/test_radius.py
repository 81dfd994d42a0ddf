"""RADIUS tests: codec, client auth/acct against an in-process server,
accounting persistence/orphan recovery, CoA, policy manager
(ref pkg/radius/*_test.go; 87.1% coverage noted in CHANGELOG.md:31)."""
import os
import socket
import time

import pytest

from bng_amd.radius import packet as rp
from bng_amd.radius.accounting import AccountingManager
from bng_amd.radius.client import Client, RadiusTimeout
from bng_amd.radius.coa import CoAProcessor, CoAServer, send_coa
from bng_amd.radius.policy import Policy, PolicyManager
from bng_amd.radius.server import RadiusServer

SECRET = b"s3cr3t"


class TestCodec:
    def test_roundtrip(self):
        p = rp.Packet(rp.ACCESS_REQUEST, 7, rp.random_authenticator())
        p.add(rp.USER_NAME, "alice").add(rp.NAS_PORT, 42)
        q = rp.Packet.decode(p.encode())
        assert q.code == 1 and q.identifier == 7
        assert q.get_str(rp.USER_NAME) == "alice"
        assert q.get_int(rp.NAS_PORT) == 42

    def test_password_encryption_roundtrip(self):
        ra = rp.random_authenticator()
        for pw in (b"x", b"exactly16bytes!!", b"longer than sixteen bytes"):
            enc = rp.encrypt_user_password(pw, SECRET, ra)
            assert len(enc) % 16 == 0
            assert rp.decrypt_user_password(enc, SECRET, ra) == pw

    def test_message_authenticator(self):
        p = rp.Packet(rp.ACCESS_REQUEST, 1, rp.random_authenticator())
        p.add(rp.USER_NAME, "bob")
        rp.sign_message_authenticator(p, SECRET)
        assert rp.verify_message_authenticator(p, SECRET)
        assert not rp.verify_message_authenticator(p, b"wrong")

    def test_response_authenticator(self):
        ra = rp.random_authenticator()
        resp = rp.Packet(rp.ACCESS_ACCEPT, 9)
        raw = rp.sign_response(resp, ra, SECRET)
        assert rp.verify_response(raw, ra, SECRET)
        assert not rp.verify_response(raw, rp.random_authenticator(), SECRET)


@pytest.fixture
def server():
    srv = RadiusServer(SECRET, users={
        "alice": {"password": "pw1", "framed_ip": "10.0.1.50",
                  "policy": "gold", "session_timeout": 3600},
        "bob": {"password": "pw2"},
    }).start()
    yield srv
    srv.stop()


class TestClient:
    def test_accept_with_attributes(self, server):
        c = Client([server.addr], SECRET)
        res = c.authenticate("alice", "pw1", mac="aa:bb:cc:00:00:01")
        assert res.success
        assert res.framed_ip == "10.0.1.50"
        assert res.policy_name == "gold"
        assert res.session_timeout == 3600
        # server saw the MAC as Calling-Station-Id
        req = server.auth_requests[-1]
        assert req.get_str(rp.CALLING_STATION_ID) == "aa:bb:cc:00:00:01"

    def test_reject_wrong_password(self, server):
        c = Client([server.addr], SECRET)
        res = c.authenticate("alice", "nope")
        assert not res.success
        assert c.stats["auth_reject"] == 1

    def test_timeout_raises(self):
        c = Client(["127.0.0.1:1"], SECRET, timeout=0.2, retries=1)
        with pytest.raises(RadiusTimeout):
            c.authenticate("alice", "pw1")

    def test_failover_rotation(self, server):
        c = Client(["127.0.0.1:1", server.addr], SECRET, timeout=0.2,
                   retries=1)
        res = c.authenticate("alice", "pw1")
        assert res.success
        # dead server rotated to the back (ref client.go:391-403)
        assert c.servers[0] == server.addr

    def test_accounting_roundtrip(self, server):
        c = Client([server.addr], SECRET)
        assert c.send_accounting(rp.ACCT_START, "sess-1", "alice",
                                 "10.0.1.50")
        assert c.send_accounting(rp.ACCT_STOP, "sess-1", "alice",
                                 "10.0.1.50", 100, 200, 60, 1)
        types = [r.get_int(rp.ACCT_STATUS_TYPE)
                 for r in server.acct_records]
        assert types == [rp.ACCT_START, rp.ACCT_STOP]
        stop = server.acct_records[-1]
        assert stop.get_int(rp.ACCT_INPUT_OCTETS) == 100
        assert stop.get_int(rp.ACCT_SESSION_TIME) == 60


class TestAccountingManager:
    def test_interim_and_stop(self, server):
        c = Client([server.addr], SECRET)
        m = AccountingManager(c, interim_interval=0.3).start()
        sid = m.start_session("alice", framed_ip="10.0.1.50")
        m.update_counters(sid, 1000, 2000)
        time.sleep(0.6)
        m.stop_session(sid)
        m.stop()
        types = [r.get_int(rp.ACCT_STATUS_TYPE)
                 for r in server.acct_records]
        assert types[0] == rp.ACCT_START
        assert rp.ACCT_INTERIM in types
        assert types[-1] == rp.ACCT_STOP

    def test_no_interim_after_the_stop(self):
        """The interim thread picks its due records and sends them
        afterwards; a session stopped in between must not get an
        Interim-Update behind its Stop.  And a Stop issued while an
        Interim-Update of that session is on the wire goes out after it."""
        import threading

        class Wire:
            def __init__(self):
                self.sent, self.hold = [], threading.Event()
                self.in_interim = threading.Event()

            def send_accounting(self, status, sid, *a, **kw):
                if status == rp.ACCT_INTERIM:
                    self.in_interim.set()
                    assert self.hold.wait(10)
                self.sent.append((status, sid))
                return True

        w = Wire()
        w.hold.set()
        m = AccountingManager(w, interim_interval=3600)
        sid = m.start_session("alice", session_id="s1")
        picked = m.sessions[sid]             # what the interim loop holds
        m.stop_session(sid)
        m._send_interim(picked)
        assert w.sent == [(rp.ACCT_START, "s1"), (rp.ACCT_STOP, "s1")]
        assert not m.send_interim(sid)

        w = Wire()
        m = AccountingManager(w, interim_interval=3600)
        sid = m.start_session("bob", session_id="s2")
        t1 = threading.Thread(target=m.send_interim, args=(sid,))
        t1.start()
        assert w.in_interim.wait(10)         # the interim is on the wire
        t2 = threading.Thread(target=m.stop_session, args=(sid,))
        t2.start()
        w.hold.set()
        t1.join(10)
        t2.join(10)
        assert w.sent == [(rp.ACCT_START, "s2"), (rp.ACCT_INTERIM, "s2"),
                          (rp.ACCT_STOP, "s2")]

    def test_pending_retry_after_partition(self, server):
        c = Client([server.addr], SECRET, timeout=0.2, retries=1)
        m = AccountingManager(c, interim_interval=3600,
                              retry_interval=3600)
        server.drop_requests = True          # partition
        m.start_session("alice", session_id="sess-p")
        assert len(m.pending) == 1
        server.drop_requests = False         # heal
        assert m.flush_pending() == 1
        assert m.pending == []
        m.stop()

    def test_orphan_recovery(self, server, tmp_path):
        path = str(tmp_path / "acct.json")
        c = Client([server.addr], SECRET)
        m1 = AccountingManager(c, persist_path=path, interim_interval=3600)
        m1.start_session("alice", session_id="orphan-1")
        # crash without stop_session; new manager recovers the orphan
        m2 = AccountingManager(c, persist_path=path, interim_interval=3600)
        assert any(p["rec"]["session_id"] == "orphan-1" and
                   p["status"] == rp.ACCT_STOP for p in m2.pending)
        assert m2.flush_pending() >= 1
        stop = server.acct_records[-1]
        assert stop.get_str(rp.ACCT_SESSION_ID) == "orphan-1"


class TestCoA:
    def test_disconnect_flow(self):
        sessions = {"sess-1": {"user": "alice", "terminated": False}}

        def lookup(req):
            return sessions.get(req.session_id)

        def terminate(s):
            s["terminated"] = True
            return True

        proc = CoAProcessor(lookup, terminate)
        srv = CoAServer(SECRET, handler=proc).start()
        try:
            code = send_coa(f"127.0.0.1:{srv.port}", SECRET,
                            rp.DISCONNECT_REQUEST, session_id="sess-1")
            assert code == rp.DISCONNECT_ACK
            assert sessions["sess-1"]["terminated"]
            code = send_coa(f"127.0.0.1:{srv.port}", SECRET,
                            rp.DISCONNECT_REQUEST, session_id="nope")
            assert code == rp.DISCONNECT_NAK
        finally:
            srv.stop()

    def test_coa_policy_update_hits_qos_hook(self):
        """CoA Filter-Id triggers the QoS table updater (the reference's
        eBPF QoS updater hook, coa_handler.go:61)."""
        updates = []
        proc = CoAProcessor(lambda r: {"ip": "10.0.1.50"},
                            lambda s: True,
                            qos_updater=lambda s, p: updates.append(p) or True)
        srv = CoAServer(SECRET, handler=proc).start()
        try:
            code = send_coa(f"127.0.0.1:{srv.port}", SECRET, rp.COA_REQUEST,
                            session_id="sess-1", policy_name="silver")
            assert code == rp.COA_ACK
            assert updates == ["silver"]
        finally:
            srv.stop()

    def test_bad_authenticator_ignored(self):
        srv = CoAServer(SECRET, handler=lambda r: (True, 0)).start()
        try:
            code = send_coa(f"127.0.0.1:{srv.port}", b"wrong-secret",
                            rp.DISCONNECT_REQUEST, session_id="x")
            assert code is None
            assert srv.stats["bad_auth"] == 1
        finally:
            srv.stop()


class TestPolicyManager:
    def test_lookup_and_default(self):
        pm = PolicyManager(default_policy=Policy("default", 10**7, 10**6))
        pm.add_policy(Policy("gold", 10**9, 10**8))
        assert pm.get("gold").download_rate_bps == 10**9
        assert pm.get("unknown").name == "default"

    def test_burst_defaults(self):
        p = Policy("x", 8 * 10**6, 8 * 10**5)
        assert p.download_burst == 10**6
        assert p.upload_burst == 100_000 or p.upload_burst == 65536 * 2 or \
            p.upload_burst == max(10**5, 65536)

    def test_from_config_and_listeners(self):
        pm = PolicyManager.from_config(
            [{"name": "basic", "download_mbps": 100, "upload_mbps": 20}],
            default="basic")
        assert pm.get("whatever").download_rate_bps == 100_000_000
        seen = []
        pm.on_change(lambda p: seen.append(p.name))
        pm.add_policy(Policy("new", 1, 1))
        assert seen == ["new"]


class TestCounterFetcher:
    """Dataplane counter pull into accounting records (ref
    accounting SetCounterFetcher tests)."""

    def test_stop_record_carries_fetched_counters(self, server):
        c = Client([server.addr], SECRET)
        am = AccountingManager(c, interim_interval=9999)
        am.set_counter_fetcher(lambda rec: (111_000, 222_000))
        sid = am.start_session("alice", framed_ip="10.0.1.5")
        am.stop_session(sid)
        stop = server.acct_records[-1]
        assert stop.get_int(rp.ACCT_STATUS_TYPE) == rp.ACCT_STOP
        assert stop.get_int(rp.ACCT_INPUT_OCTETS) == 111_000
        assert stop.get_int(rp.ACCT_OUTPUT_OCTETS) == 222_000

    def test_fetcher_errors_keep_pushed_values(self, server):
        c = Client([server.addr], SECRET)
        am = AccountingManager(c, interim_interval=9999)

        def boom(rec):
            raise RuntimeError("dataplane gone")
        am.set_counter_fetcher(boom)
        sid = am.start_session("bob")
        am.update_counters(sid, 10, 20)
        am.stop_session(sid)
        stop = server.acct_records[-1]
        assert stop.get_int(rp.ACCT_INPUT_OCTETS) == 10
        assert stop.get_int(rp.ACCT_OUTPUT_OCTETS) == 20


class TestPacketFuzz:
    """Codec robustness on adversarial bytes (ref pkg/dhcp/fuzz_test.go
    strategy applied to the RADIUS codec)."""

    def test_random_bytes_never_crash(self):
        import random
        rng = random.Random(1234)
        parsed = 0
        for _ in range(2000):
            n = rng.randrange(0, 64)
            raw = bytes(rng.randrange(256) for _ in range(n))
            try:
                p = rp.Packet.decode(raw)
                parsed += 1
                assert 0 <= p.code <= 255
            except (rp.RadiusError, ValueError, IndexError):
                pass
        # truncated/garbled real packet prefixes
        req = rp.Packet(rp.ACCESS_REQUEST, 1, rp.random_authenticator())
        req.add(rp.USER_NAME, "alice")
        raw = req.encode()
        for cut in range(len(raw)):
            try:
                rp.Packet.decode(raw[:cut])
            except (rp.RadiusError, ValueError, IndexError):
                pass
        for flip in range(0, len(raw), 3):
            mutated = bytearray(raw)
            mutated[flip] ^= 0xFF
            try:
                rp.Packet.decode(bytes(mutated))
            except (rp.RadiusError, ValueError, IndexError):
                pass


class TestMessageAuthenticatorVerification:
    """Round-1 advisor: verify Message-Authenticator on Access
    responses (blast-RADIUS / CVE-2024-3596 client-side mitigation)."""

    def _srv(self):
        srv = RadiusServer(b"s3cret",
                           users={"alice": {"password": "pw1"}})
        srv.start()
        return srv

    def test_response_carries_and_verifies_ma(self):
        srv = self._srv()
        try:
            c = Client([f"127.0.0.1:{srv.port}"], b"s3cret",
                       require_message_authenticator=True)
            res = c.authenticate("alice", "pw1")
            assert res.success
            assert c.stats["ma_invalid"] == 0
            assert c.stats["ma_missing"] == 0
        finally:
            srv.stop()

    def test_forged_response_dropped(self):
        """A response whose MA is tampered must be treated as forged
        (dropped), not accepted."""
        import socket as _s
        import threading as _t
        from bng_amd.radius import packet as rp

        sock = _s.socket(_s.AF_INET, _s.SOCK_DGRAM)
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
        secret = b"s3cret"

        def forger():
            data, addr = sock.recvfrom(4096)
            req = rp.Packet.decode(data)
            resp = rp.Packet(rp.ACCESS_ACCEPT, req.identifier)
            raw = rp.sign_response_with_ma(resp, req.authenticator, secret)
            # tamper with the MA bytes but keep the Response
            # Authenticator valid for the tampered attrs (the attack:
            # MD5 response-auth forgery with bogus MA)
            resp2 = rp.Packet.decode(raw)
            resp2.attributes = [
                (t, b"\x00" * 16 if t == rp.MESSAGE_AUTHENTICATOR else v)
                for t, v in resp2.attributes]
            raw2 = rp.sign_response(resp2, req.authenticator, secret)
            sock.sendto(raw2, addr)

        th = _t.Thread(target=forger, daemon=True)
        th.start()
        c = Client([f"127.0.0.1:{port}"], secret, retries=1, timeout=0.5)
        with pytest.raises(RadiusTimeout):
            c.authenticate("alice", "pw1")
        assert c.stats["ma_invalid"] == 1
        sock.close()

    def test_require_ma_rejects_bare_response(self):
        import socket as _s
        import threading as _t
        from bng_amd.radius import packet as rp

        sock = _s.socket(_s.AF_INET, _s.SOCK_DGRAM)
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
        secret = b"s3cret"

        def bare():
            data, addr = sock.recvfrom(4096)
            req = rp.Packet.decode(data)
            resp = rp.Packet(rp.ACCESS_ACCEPT, req.identifier)
            sock.sendto(rp.sign_response(resp, req.authenticator, secret),
                        addr)

        _t.Thread(target=bare, daemon=True).start()
        c = Client([f"127.0.0.1:{port}"], secret, retries=1, timeout=0.5,
                   require_message_authenticator=True)
        with pytest.raises(RadiusTimeout):
            c.authenticate("alice", "pw1")
        assert c.stats["ma_missing"] >= 1
        sock.close()
