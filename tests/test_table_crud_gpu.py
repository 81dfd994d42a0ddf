"""Table-management kernels (the BPF-map-update analog) on tiny tables.

The extension derives a table's slot count from the tensor's byte size, so
every test builds its own 128-slot tables (128 = BNG_MAX_PROBE: one chain
covers the whole table) and calls ext.* directly.

Oracle: a pure-Python model of the two table kinds, exact to the byte.
  * KeyTable — 64-bit key at offset 0, empty = 0, tombstone = all ones; an
    upsert takes the first tombstone of its chain, but only once an empty
    slot proves the key absent (subscriber, binding, PPPoE by-IP);
  * IpTable  — 32-bit key at offset 0, empty = 0, no tombstones (subscriber
    context, egress QoS).
Sequential scripts (one record per launch) are compared byte for byte with
the model's image.  In-batch races place keys nondeterministically, so the
batch tests assert the placement invariants instead.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bng_amd.dataplane import abi

SLOTS = 128
assert SLOTS == abi.MAX_PROBE
TOMB = abi.KEY_TOMBSTONE


# ------------------------------------------------------------------ model
class KeyTable:
    def __init__(self, size, slots=SLOTS):
        self.size, self.n = size, slots
        self.img = bytearray(size * slots)

    def key(self, s):
        return int.from_bytes(self.img[s * self.size:s * self.size + 8],
                              "little")

    def _chain(self, key):
        home = abi.mix64(key) & (self.n - 1)
        return [(home + i) & (self.n - 1) for i in range(abi.MAX_PROBE)]

    def find(self, key):
        for s in self._chain(key):
            if self.key(s) == key:
                return s
            if self.key(s) == 0:
                return None
        return None

    def upsert(self, rec: bytes) -> int:
        key, tomb = int.from_bytes(rec[:8], "little"), None
        for s in self._chain(key):
            cur = self.key(s)
            if cur == TOMB and tomb is None:
                tomb = s
            if cur == key or cur == 0:
                if cur == 0 and tomb is not None:
                    s = tomb
                self.img[s * self.size:(s + 1) * self.size] = rec
                return 0
        return -1

    def delete(self, key):
        s = self.find(key)
        if s is not None:
            self.img[s * self.size:s * self.size + 8] = b"\xff" * 8


class IpTable:
    def __init__(self, cls, slots=SLOTS):
        self.cls, self.size, self.n = cls, ctypes.sizeof(cls), slots
        self.img = bytearray(self.size * slots)

    def entry(self, s):
        return self.cls.from_buffer(self.img, s * self.size)

    def slot(self, ip, claim=True):
        """Entry that carries `ip` (claimed if absent and `claim`), None
        when absent and not claimed, -1 when the chain is full."""
        home = abi.mix64(ip) & (self.n - 1)
        for i in range(abi.MAX_PROBE):
            e = self.entry((home + i) & (self.n - 1))
            if e.key_ip == 0:
                if not claim:
                    return None
                e.key_ip = ip
            if e.key_ip == ip:
                return e
        return -1


def apply_subctx(e, r, um):
    if um & abi.CTX_SET_NAT:
        for f in ("public_ip", "port_start", "port_end", "next_port",
                  "subscriber_id", "flags"):
            setattr(e, f, getattr(r, f))
        e.nat_valid = 1
    if um & abi.CTX_SET_QOS:
        for f in ("rate_bps", "tokens", "last_update", "burst_bytes",
                  "priority"):
            setattr(e, f, getattr(r, f))
        e.qos_valid = 1
    if um & abi.CTX_CLR_QOS:
        e.qos_valid = 0
    if um & abi.CTX_CLR_NAT:
        e.nat_valid = 0


def apply_qos(e, r, _um=0):
    for f in ("rate_bps", "tokens", "last_update", "burst_bytes", "priority",
              "valid"):
        setattr(e, f, getattr(r, f))


# ---------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def ext():
    from bng_amd.dataplane.build import get_ext
    return get_ext(required=True)


def dev(raw):
    import torch
    return torch.from_numpy(np.frombuffer(bytearray(raw), dtype=np.uint8)) \
        .cuda()


def zeros(nbytes):
    import torch
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


def rc_of(n):
    import torch
    return torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")


def image(t) -> bytes:
    return t.cpu().numpy().tobytes()


def keys_dev(keys, dtype=np.uint64):
    import torch
    return torch.from_numpy(
        np.array(keys, dtype=dtype).view(np.int64 if dtype == np.uint64
                                         else np.int32)).cuda()


def raw(s) -> bytes:
    return ctypes.string_at(ctypes.addressof(s), ctypes.sizeof(s))


def colliding(key_of, count, start=0):
    """`count` indices i >= start whose key_of(i) share one home slot."""
    homes = {}
    i = start
    while True:
        g = homes.setdefault(abi.mix64(key_of(i)) & (SLOTS - 1), [])
        g.append(i)
        if len(g) == count:
            return g
        i += 1


# --------------------------------------- drivers of the 64-bit-key tables
class SubDriver:
    """Subscriber table: ext.sub_upsert / ext.sub_delete."""
    size = 32

    def __init__(self, ext):
        self.ext, self.t = ext, zeros(SLOTS * 32)
        self.model = KeyTable(32)

    @staticmethod
    def key(i):
        return 0xAA0000000000 + i

    def rec(self, i, v=0):
        return raw(abi.SubEntry(
            key=self.key(i), pool_id=1 + v, allocated_ip=0x0A000001 + i + v,
            lease_expiry=1_700_000_000 + 1000 * v + i, vlan_id=100 + v,
            client_class=v & 0xFF, flags=(i + v) & 0xFF))

    def upsert(self, items):
        """items: (i, v) pairs, one launch.  Returns rc as a list."""
        rc = rc_of(len(items))
        self.ext.sub_upsert(self.t, dev(b"".join(self.rec(*x)
                                                 for x in items)), rc)
        return rc.cpu().tolist()[:len(items)]

    def model_upsert(self, i, v=0):
        return self.model.upsert(self.rec(i, v))

    def delete(self, i):
        self.ext.sub_delete(self.t, keys_dev([self.key(i)]))
        self.model.delete(self.key(i))

    def table_image(self):
        return image(self.t)


class BindingDriver(SubDriver):
    """Antispoof binding table: ext.binding_upsert / ext.binding_delete."""

    @staticmethod
    def key(i):
        return 0x02BB00000000 + 3 * i

    def rec(self, i, v=0):
        b = abi.BindingEntry(key_mac=self.key(i), ipv4_addr=0x0A010001 + i,
                             ipv4_valid=1, ipv6_valid=v & 1,
                             mode=abi.AS_STRICT + (v & 1))
        for j in range(16):
            b.ipv6_addr[j] = (i + 17 * j + v) & 0xFF
        return raw(b)

    def upsert(self, items):
        rc = rc_of(len(items))
        self.ext.binding_upsert(self.t, dev(b"".join(self.rec(*x)
                                                     for x in items)), rc)
        return rc.cpu().tolist()[:len(items)]

    def delete(self, i):
        self.ext.binding_delete(self.t, keys_dev([self.key(i)]))
        self.model.delete(self.key(i))


class PppoeDriver:
    """PPPoE by-IP table, driven through pppoe_sess_upsert / _delete.
    Index i names both the subscriber address and the session id."""
    size = 16

    def __init__(self, ext):
        self.ext, self.t = ext, zeros(SLOTS * 16)
        self.sess = zeros(abi.PPPOE_MAX_SESSIONS * 16)
        self.model = KeyTable(16)
        self.msess = bytearray(abi.PPPOE_MAX_SESSIONS * 16)

    @staticmethod
    def ip(i):
        return 0x0A020001 + i

    @classmethod
    def key(cls, i):
        return abi.pppoe_ip_key(cls.ip(i))

    @staticmethod
    def sid(i):
        return (i * 61 + 1) & 0xFFFF

    @staticmethod
    def mac(i, v):
        return 0xAABBCC000000 + (v << 16) + i

    def sess_rec(self, i, v=0):
        return raw(abi.PppoeSess(mac_valid=self.mac(i, v), ip=self.ip(i),
                                 mru=1492 - v, session_id=self.sid(i)))

    def rec(self, i, v=0):
        return raw(abi.PppoeIp(key=self.key(i),
                               sid_mac=(self.sid(i) << 48) | self.mac(i, v)))

    def upsert(self, items):
        rc = rc_of(len(items))
        self.ext.pppoe_sess_upsert(
            self.sess, self.t,
            dev(b"".join(self.sess_rec(*x) for x in items)), rc)
        return rc.cpu().tolist()[:len(items)]

    def _msess(self, sid):
        return abi.PppoeSess.from_buffer(self.msess, sid * 16)

    def model_upsert(self, i, v=0):
        s = self._msess(self.sid(i))
        r = self.model.upsert(self.rec(i, v))
        if r == 0:
            s.mac_valid = self.mac(i, v) | abi.PPPOE_VALID
            s.ip, s.mru, s.session_id = self.ip(i), 1492 - v, self.sid(i)
        else:
            s.mac_valid = s.ip = s.mru = s.session_id = 0
        return r

    def delete(self, i):
        self.ext.pppoe_sess_delete(self.sess, self.t,
                                   keys_dev([self.sid(i)], np.int32))
        s = self._msess(self.sid(i))
        if s.mac_valid & abi.PPPOE_VALID:
            self.model.delete(abi.pppoe_ip_key(s.ip))
            s.mac_valid = s.ip = s.mru = s.session_id = 0

    def table_image(self):
        return image(self.t)


DRIVERS = [SubDriver, BindingDriver, PppoeDriver]


def parse_keys(img, size, width=8):
    return [int.from_bytes(img[s * size:s * size + width], "little")
            for s in range(len(img) // size)]


def check_placement(img, size, want, width=8):
    """`want` maps key -> full entry bytes.  Every key sits in exactly one
    slot, reachable from its home slot without crossing an empty one, with
    its value; every other slot is all zero."""
    keys = parse_keys(img, size, width)
    n = len(keys)
    assert sorted(k for k in keys if k) == sorted(want)
    for s, k in enumerate(keys):
        ent = img[s * size:(s + 1) * size]
        if k == 0:
            assert ent == bytes(size), f"slot {s} not clean"
            continue
        assert ent == want[k], f"slot {s} value mismatch"
        home = abi.mix64(k) & (n - 1)
        for d in range((s - home) % n):
            assert keys[(home + d) % n] != 0, \
                f"key {k:#x} at {s} is behind an empty slot"


# ------------------------------------------------- 64-bit-key table tests
@pytest.mark.parametrize("drv", DRIVERS, ids=lambda d: d.__name__)
class TestKeyTables:
    def test_sequential_script(self, ext, drv):
        """Insert (with a chain of four keys on one home slot), overwrite,
        delete mid-chain, delete absent, re-insert into the tombstone, add
        more colliding keys: image equals the model's, all rc 0.  Seven
        keys in 128 slots: every chain walked ends at an empty slot."""
        import torch
        d = drv(ext)
        a = colliding(d.key, 5)
        others = [2000, 2001, 2002]
        assert max(a) < 2000
        slot_of = lambda i: d.model.find(d.key(i))

        def up(i, v=0):
            assert d.upsert([(i, v)]) == [0]
            assert d.model_upsert(i, v) == 0

        up(a[0]); up(others[0]); up(a[1]); up(a[2]); up(others[1])
        up(a[1], 5)                          # overwrite
        mid = slot_of(a[1])
        assert slot_of(a[0]) != mid != slot_of(a[2])
        d.delete(a[1])                       # middle of the chain
        assert d.model.key(mid) == TOMB and slot_of(a[2]) is not None
        d.delete(2999)                       # absent
        up(a[1], 9)                          # re-insert: takes the tombstone
        assert slot_of(a[1]) == mid
        up(a[3])                             # new colliding key: chain end
        head = slot_of(a[0])
        d.delete(a[0])                       # head of the chain
        up(a[4], 2)                          # new key reuses the tombstone
        assert slot_of(a[4]) == head
        up(others[2])
        torch.cuda.synchronize()
        assert d.table_image() == bytes(d.model.img)
        if drv is PppoeDriver:
            assert image(d.sess) == bytes(d.msess)

    def test_chain_full(self, ext, drv):
        d = drv(ext)
        items = [(i, 0) for i in range(SLOTS)]
        assert d.upsert(items) == [0] * SLOTS
        full = d.table_image()
        assert 0 not in parse_keys(full, d.size)
        # one more distinct key: rc -1, nothing written
        assert d.upsert([(SLOTS, 0)]) == [-1]
        assert d.table_image() == full
        if drv is PppoeDriver:
            sid = d.sid(SLOTS)
            assert image(d.sess)[sid * 16:sid * 16 + 16] == bytes(16)
        # overwrite of a present key still succeeds, in place
        assert d.upsert([(5, 3)]) == [0]
        after = d.table_image()
        s = parse_keys(full, d.size).index(d.key(5))
        assert after[s * d.size:(s + 1) * d.size] == d.rec(5, 3)
        assert after[:s * d.size] == full[:s * d.size]
        assert after[(s + 1) * d.size:] == full[(s + 1) * d.size:]

    def test_batch_fills_table(self, ext, drv):
        """128 distinct keys race for 128 slots in one launch."""
        d = drv(ext)
        assert d.upsert([(i, 1) for i in range(SLOTS)]) == [0] * SLOTS
        check_placement(d.table_image(), d.size,
                        {d.key(i): d.rec(i, 1) for i in range(SLOTS)})

    def test_batch_overflows_table(self, ext, drv):
        """256 distinct keys, 128 slots: a thread visits each slot once and
        gives up only after seeing all of them taken, so exactly 128 win."""
        d = drv(ext)
        n = 2 * SLOTS
        rc = d.upsert([(i, 1) for i in range(n)])
        assert sorted(set(rc)) == [-1, 0]
        won = [i for i in range(n) if rc[i] == 0]
        assert len(won) == SLOTS
        check_placement(d.table_image(), d.size,
                        {d.key(i): d.rec(i, 1) for i in won})
        if drv is PppoeDriver:
            simg = image(d.sess)
            for i in range(n):
                e = abi.PppoeSess.from_buffer_copy(simg, d.sid(i) * 16)
                assert bool(e.mac_valid & abi.PPPOE_VALID) == (rc[i] == 0)


# ------------------------------------------------- 32-bit-key table tests
def ctx_rec(ip, v=0):
    return abi.SubCtx(key_ip=ip, public_ip=0xCB007100 + v, port_start=1024,
                      port_end=2047, next_port=1024 + v, subscriber_id=ip & 0xFFFF,
                      flags=v & 0xFF, priority=v & 7, rate_bps=10**9 + v,
                      tokens=1 << 20, last_update=1_700_000_000 * 10**9 + v,
                      burst_bytes=(1 << 20) + v)


def qos_rec(ip, v=0, valid=1):
    return abi.QosBucket(key_ip=ip, valid=valid, priority=v & 7,
                         rate_bps=10**8 + v, tokens=(1 << 18) + v,
                         last_update=1_700_000_000 * 10**9 + v,
                         burst_bytes=(1 << 18) + v)


class CtxDriver:
    cls, apply = abi.SubCtx, staticmethod(apply_subctx)
    rec = staticmethod(ctx_rec)
    batch_um = abi.CTX_SET_NAT | abi.CTX_SET_QOS

    def __init__(self, ext):
        self.ext, self.t = ext, zeros(SLOTS * 64)
        self.model = IpTable(self.cls)

    def launch(self, recs, um, rc):
        self.ext.subctx_upsert(self.t, dev(b"".join(map(raw, recs))), um, rc)

    def upsert(self, recs, um):
        rc = rc_of(len(recs))
        self.launch(recs, um, rc)
        return rc.cpu().tolist()[:len(recs)]

    def claims(self, um):
        return bool(um & (abi.CTX_SET_NAT | abi.CTX_SET_QOS))

    def step(self, r, um=0):
        """One record on the device and in the model; returns the model's
        entry (None when nothing was claimed)."""
        assert self.upsert([r], um) == [0]
        e = self.model.slot(r.key_ip, self.claims(um))
        assert e != -1
        if e is not None:
            self.apply(e, r, um)
        return e

    def expected(self, r):
        e = self.cls(key_ip=r.key_ip)
        self.apply(e, r, self.batch_um)
        return raw(e)


class QosDriver(CtxDriver):
    cls, apply = abi.QosBucket, staticmethod(apply_qos)
    rec = staticmethod(qos_rec)
    batch_um = 0

    def launch(self, recs, um, rc):
        self.ext.qos_upsert(self.t, dev(b"".join(map(raw, recs))), rc)

    def claims(self, um):
        return True


def ip_of(i):
    return 0x0A030001 + i


class TestIpTables:
    def test_subctx_script(self, ext):
        import torch
        d = CtxDriver(ext)
        a = colliding(ip_of, 3)
        # a clear of an absent key claims nothing
        assert d.step(ctx_rec(ip_of(a[0])), abi.CTX_CLR_QOS) is None
        torch.cuda.synchronize()
        assert image(d.t) == bytes(SLOTS * 64)
        # NAT half then QoS half of one key: both kept
        d.step(ctx_rec(ip_of(a[0]), 1), abi.CTX_SET_NAT)
        e = d.step(ctx_rec(ip_of(a[0]), 2), abi.CTX_SET_QOS)
        assert (e.nat_valid, e.qos_valid) == (1, 1)
        assert (e.next_port, e.rate_bps) == (1025, 10**9 + 2)
        d.step(ctx_rec(ip_of(a[1]), 3), abi.CTX_SET_QOS)    # collides
        d.step(ctx_rec(ip_of(a[2]), 4), abi.CTX_SET_NAT | abi.CTX_SET_QOS)
        d.step(ctx_rec(ip_of(a[1]), 5), abi.CTX_SET_NAT)    # merge, 2nd slot
        d.step(ctx_rec(ip_of(a[0])), abi.CTX_CLR_QOS)
        d.step(ctx_rec(ip_of(a[2])), abi.CTX_CLR_NAT)
        d.step(ctx_rec(ip_of(5000), 6), abi.CTX_SET_NAT)
        d.step(ctx_rec(ip_of(5001)), abi.CTX_CLR_NAT)       # absent again
        torch.cuda.synchronize()
        assert image(d.t) == bytes(d.model.img)

    def test_qos_script(self, ext):
        import torch
        d = QosDriver(ext)
        a = colliding(ip_of, 3)
        # valid=0 on an absent key does claim a slot
        e = d.step(qos_rec(ip_of(a[0]), 1, valid=0))
        assert (e.key_ip, e.valid) == (ip_of(a[0]), 0)
        d.step(qos_rec(ip_of(a[1]), 2))                     # collides
        d.step(qos_rec(ip_of(a[0]), 3))                     # overwrite
        d.step(qos_rec(ip_of(a[2]), 4))
        d.step(qos_rec(ip_of(a[1]), 5, valid=0))            # remove policy
        d.step(qos_rec(ip_of(5000), 6))
        torch.cuda.synchronize()
        img = image(d.t)
        assert img == bytes(d.model.img)
        assert sum(1 for k in parse_keys(img, 64, 4) if k) == 4

    @pytest.mark.parametrize("drv", [CtxDriver, QosDriver],
                             ids=lambda d: d.__name__)
    def test_batch_fills_table(self, ext, drv):
        d = drv(ext)
        recs = [d.rec(ip_of(i), i) for i in range(SLOTS)]
        assert d.upsert(recs, d.batch_um) == [0] * SLOTS
        check_placement(image(d.t), 64,
                        {r.key_ip: d.expected(r) for r in recs}, width=4)

    @pytest.mark.parametrize("drv", [CtxDriver, QosDriver],
                             ids=lambda d: d.__name__)
    def test_batch_overflows_table(self, ext, drv):
        d = drv(ext)
        recs = [d.rec(ip_of(i), i) for i in range(2 * SLOTS)]
        rc = d.upsert(recs, d.batch_um)
        assert sorted(set(rc)) == [-1, 0]
        won = [r for r, c in zip(recs, rc) if c == 0]
        assert len(won) == SLOTS
        check_placement(image(d.t), 64,
                        {r.key_ip: d.expected(r) for r in won}, width=4)


# ------------------------------------------------------------ sess_import
def probe(img, cls, sig):
    """Entry of a sig table (home = low bits of sig) or None."""
    size = ctypes.sizeof(cls)
    n = len(img) // size
    for i in range(abi.MAX_PROBE):
        e = cls.from_buffer_copy(img, ((sig + i) & (n - 1)) * size)
        if e.sig == sig:
            return e
        if e.sig == 0:
            return None
    return None


def tup(t):
    return (t.src_ip, t.dst_ip, t.src_port, t.dst_port, t.protocol)


def test_sess_import(ext):
    import torch
    n_slots = 256
    sess, rev, eim = (zeros(n_slots * 128), zeros(n_slots * 48),
                      zeros(n_slots * 48))
    recs = np.zeros(7, dtype=abi.SESS_EXPORT_DTYPE)
    for i in range(len(recs)):
        recs[i] = (0x0A000010 + i, 0x5DB8D822 + 3 * i, 40000 + i, 53 + i,
                   (17, 6, 1)[i % 3], abi.NAT_ESTABLISHED if i % 2 else
                   abi.NAT_NEW, i == 5, i % 2, 0xCB007101, 2000 + i,
                   (3000 + i) if i % 2 else 0, 10**18 + i, 10**18 + 50 + i, 0)
    rc = torch.zeros(len(recs), dtype=torch.int32, device="cuda")
    ext.sess_import(sess, rev, eim,
                    torch.from_numpy(recs.view(np.uint8)).cuda().flatten(), rc)
    assert rc.cpu().tolist() == [0] * len(recs)
    simg, rimg, eimg = image(sess), image(rev), image(eim)
    n_eim = 0
    for r in recs:
        r = {f: int(r[f]) for f in recs.dtype.names}
        key = (r["src_ip"], r["dst_ip"], r["src_port"], r["dst_port"],
               r["protocol"])
        s = probe(simg, abi.NatSession, abi.tuple_sig(*key))
        assert s is not None and s.ready == 1 and tup(s.key) == key
        assert (s.nat_ip, s.nat_port, s.orig_ip, s.orig_port) == \
            (r["nat_ip"], r["nat_port"], r["src_ip"], r["src_port"])
        assert (s.state, s.is_hairpin, s.last_seen, s.created) == \
            (r["state"], r["is_hairpin"], r["last_seen"], r["created"])
        assert (s.packets_out, s.packets_in, s.bytes_out, s.bytes_in) == \
            (0, 0, 0, 0)
        rkey = (r["dst_ip"], r["nat_ip"], r["dst_port"], r["nat_port"],
                r["protocol"])
        v = probe(rimg, abi.NatReverse, abi.tuple_sig(*rkey))
        assert v is not None and v.ready == 1
        assert tup(v.key) == rkey and tup(v.orig) == key
        m = probe(eimg, abi.EimEntry,
                  abi.eim_sig(r["src_ip"], r["src_port"], r["protocol"]))
        if not r["flags"] & 1:
            assert m is None
            continue
        n_eim += 1
        assert m is not None and m.ready == 1
        assert (m.internal_ip, m.internal_port, m.protocol) == \
            (r["src_ip"], r["src_port"], r["protocol"])
        assert (m.external_ip, m.external_port) == \
            (r["nat_ip"], r["eim_port"])
        assert (m.created, m.last_used, m.ref_count, m.flags) == \
            (r["created"], r["last_seen"], 1, 0)
    assert n_eim == 3
    count = lambda img, size: sum(1 for k in parse_keys(img, size) if k)
    assert (count(simg, 128), count(rimg, 48), count(eimg, 48)) == (7, 7, 3)


# ------------------------------------------------- argument validation
class TestArgumentChecks:
    """The extension refuses what would index out of bounds on the device.
    None of these launches a kernel."""

    def test_short_rc(self, ext):
        import torch
        t, batch = zeros(SLOTS * 32), zeros(2 * 32)
        rc = torch.zeros(1, dtype=torch.int32, device="cuda")
        with pytest.raises(RuntimeError, match="rc must hold"):
            ext.sub_upsert(t, batch, rc)
        with pytest.raises(RuntimeError, match="rc must hold"):
            ext.binding_upsert(t, batch, rc)
        with pytest.raises(RuntimeError, match="rc must hold"):
            ext.qos_upsert(zeros(SLOTS * 64), zeros(2 * 64), rc)
        with pytest.raises(RuntimeError, match="rc must hold"):
            ext.subctx_upsert(zeros(SLOTS * 64), zeros(2 * 64),
                              abi.CTX_SET_NAT, rc)
        rc64 = torch.zeros(2, dtype=torch.int64, device="cuda")
        with pytest.raises(RuntimeError, match="rc must hold"):
            ext.sub_upsert(t, batch, rc64)

    def test_ragged_batch(self, ext):
        with pytest.raises(RuntimeError, match="whole number"):
            ext.sub_upsert(zeros(SLOTS * 32), zeros(33), rc_of(2))

    def test_int32_delete_keys(self, ext):
        keys = keys_dev([1, 2], np.int32)
        with pytest.raises(RuntimeError, match="64-bit"):
            ext.sub_delete(zeros(SLOTS * 32), keys)
        with pytest.raises(RuntimeError, match="64-bit"):
            ext.binding_delete(zeros(SLOTS * 32), keys)

    def test_host_tensor_and_table_size(self, ext):
        import torch
        host = torch.zeros(SLOTS * 32, dtype=torch.uint8)
        with pytest.raises(RuntimeError, match="device tensor"):
            ext.sub_delete(host, keys_dev([1]))
        with pytest.raises(RuntimeError, match="device tensor"):
            ext.binding_upsert(zeros(SLOTS * 32), host[:32], rc_of(1))
        with pytest.raises(RuntimeError, match="power of two"):
            ext.sub_upsert(zeros(96 * 32), zeros(32), rc_of(1))

    def test_empty_batch_returns(self, ext):
        import torch
        rc = rc_of(0)
        t32, t64 = zeros(SLOTS * 32), zeros(SLOTS * 64)
        ext.sub_upsert(t32, zeros(0), rc)
        ext.binding_upsert(t32, zeros(0), rc)
        ext.qos_upsert(t64, zeros(0), rc)
        ext.subctx_upsert(t64, zeros(0), abi.CTX_SET_NAT, rc)
        ext.sess_import(zeros(256 * 128), zeros(256 * 48), zeros(256 * 48),
                        zeros(0), rc)
        none = torch.zeros(0, dtype=torch.int64, device="cuda")
        ext.sub_delete(t32, none)
        ext.binding_delete(t32, none)
        torch.cuda.synchronize()
        assert rc.cpu().tolist() == [7]
        assert image(t32) == bytes(SLOTS * 32)
