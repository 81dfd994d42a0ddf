"""Receiver-side checks of NAT44 output, independent of the golden model.

The GPU tests compare the kernels with `GoldenDataplane`, which is a port of
the same incremental-checksum algorithm: a mistake the two share is
invisible there.  This module looks at a frame the way the host that
receives it does, and at a translation the way an auditor does, and knows
nothing of how the translator works:

  * `verify_frame` sums the IPv4 header and, where the whole datagram is in
    the frame, the TCP/UDP/ICMP message, checksum field included, and wants
    0xFFFF.  Summing over the field treats both representations of zero
    alike.
  * `verify_translation` compares a frame before and after NAT: which bytes
    may differ, what the new address and port must be, and the delta
    invariant — the ones-complement sum of everything a checksum covers is
    the same before and after, so a checksum that was right stays right
    and one that was wrong stays wrong by the same amount.  That holds
    where nothing can be summed from scratch: first fragments, and frames
    that arrived with a bad checksum.
  * `untouched` is for frames the NAT stage must leave alone.

It also builds the seeded corpus those checks run on (`corpus`), with
`struct` alone.  Nothing here imports the golden model or the project's
checksum helpers, and nothing updates a checksum incrementally: every
checksum the builders write is summed from scratch over the bytes it covers.
"""
import random
import struct
from collections import namedtuple

ETH_IP = 0x0800
TCP, UDP, ICMP = 6, 17, 1
PROTO_NAME = {TCP: "tcp", UDP: "udp", ICMP: "icmp"}
L4_HDR = {TCP: 20, UDP: 8, ICMP: 8}
#: offset of the checksum / of the translated port or id inside the L4 header
CSUM_AT = {TCP: 16, UDP: 6, ICMP: 2}
SRC_ID_AT = {TCP: 0, UDP: 0, ICMP: 4}
DST_ID_AT = {TCP: 2, UDP: 2, ICMP: 4}
ICMP_QUERIES = (0, 8, 13, 14, 15, 16, 17, 18)

GW_MAC = bytes.fromhex("020000000001")
DST_IP = 0x5DB8D822                      # 93.184.216.34


# ------------------------------------------------------------ arithmetic
def ones_sum(data) -> int:
    """Ones-complement sum of big-endian 16-bit words, an odd last byte
    padded with zero, folded to 16 bits.  0 only for all-zero data."""
    data = bytes(data)
    if len(data) & 1:
        data += b"\x00"
    s = sum(struct.unpack(">%dH" % (len(data) // 2), data))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def same_sum(a: int, b: int) -> bool:
    """Equality of folded ones-complement sums: 0x0000 and 0xFFFF are the
    two representations of zero."""
    return a % 0xFFFF == b % 0xFFFF


def _u16(b, o):
    return struct.unpack_from(">H", b, o)[0]


def _u32(b, o):
    return struct.unpack_from(">I", b, o)[0]


# ---------------------------------------------------------------- parsing
Layout = namedtuple("Layout", "ihl l4 proto total end frag_off mf whole")


def layout(frame):
    """Header geometry of an untagged IPv4 frame, or a string saying why it
    is not one.  `end` is where the IP packet ends inside the frame (the
    rest is Ethernet padding); `whole` says the frame holds a complete,
    unfragmented datagram with all of its L4 header."""
    n = len(frame)
    if n < 14 or _u16(frame, 12) != ETH_IP:
        return "not an IPv4 ethertype"
    if n < 34:
        return "too short for an IPv4 header"
    if frame[14] >> 4 != 4:
        return "IP version %d" % (frame[14] >> 4)
    ihl = (frame[14] & 0xF) * 4
    if ihl < 20:
        return "ihl %d < 5" % (ihl // 4)
    if n < 14 + ihl:
        return "IP header does not fit in the frame"
    total = _u16(frame, 16)
    ff = _u16(frame, 20)
    frag_off, mf = ff & 0x1FFF, bool(ff & 0x2000)
    proto = frame[23]
    l4 = 14 + ihl
    fits = ihl <= total and 14 + total <= n
    end = 14 + total if fits else n
    whole = (fits and frag_off == 0 and not mf and
             end - l4 >= L4_HDR.get(proto, 0))
    return Layout(ihl, l4, proto, total, end, frag_off, mf, whole)


def pseudo_header(frame, lay) -> bytes:
    return bytes(frame[26:34]) + struct.pack(">BBH", 0, lay.proto,
                                             lay.end - lay.l4)


def flow_fields(frame):
    """(src, dst, proto, source port or id, destination port or id)."""
    lay = layout(frame)
    assert not isinstance(lay, str), lay
    return (_u32(frame, 26), _u32(frame, 30), lay.proto,
            _u16(frame, lay.l4 + SRC_ID_AT[lay.proto]),
            _u16(frame, lay.l4 + DST_ID_AT[lay.proto]))


# ------------------------------------------------------------- the oracle
def verify_frame(frame) -> list:
    """What a receiving host would reject the frame for."""
    lay = layout(frame)
    if isinstance(lay, str):
        return [lay]
    bad = []
    s = ones_sum(frame[14:14 + lay.ihl])
    if s != 0xFFFF:
        bad.append("IP header sums to %#06x" % s)
    if not lay.whole or lay.proto not in L4_HDR:
        return bad
    seg = bytes(frame[lay.l4:lay.end])
    if lay.proto == ICMP:
        s = ones_sum(seg)
    elif lay.proto == UDP and _u16(frame, lay.l4 + 6) == 0:
        return bad                       # sender computed none
    else:
        s = ones_sum(pseudo_header(frame, lay) + seg)
    if s != 0xFFFF:
        bad.append("%s message sums to %#06x" % (PROTO_NAME[lay.proto], s))
    return bad


def from_scratch_possible(frame) -> bool:
    """verify_frame checks the L4 checksum of this frame, not only the
    header's."""
    lay = layout(frame)
    if isinstance(lay, str) or not lay.whole or lay.proto not in L4_HDR:
        return False
    return not (lay.proto == UDP and _u16(frame, lay.l4 + 6) == 0)


def untouched(before, after) -> list:
    before, after = bytes(before), bytes(after)
    if len(before) != len(after):
        return ["length %d became %d" % (len(before), len(after))]
    diff = [i for i in range(len(before)) if before[i] != after[i]]
    return ["bytes changed at %s" % diff[:16]] if diff else []


def verify_translation(before, after, direction, public_ip=None,
                       port_range=None) -> list:
    """`after` is a legal NAT44 translation of `before`.  direction is
    "egress" (source rewritten; the new source must be public_ip and the
    new port or id lie in port_range, both inclusive) or "ingress"
    (destination rewritten)."""
    assert direction in ("egress", "ingress")
    before, after = bytes(before), bytes(after)
    if len(before) != len(after):
        return ["length %d became %d" % (len(before), len(after))]
    lay = layout(before)
    if isinstance(lay, str):
        return ["not translatable: " + lay]
    if lay.proto not in L4_HDR or lay.frag_off or \
            len(before) < lay.l4 + L4_HDR[lay.proto]:
        return ["not translatable: no L4 header in the frame"]
    egress = direction == "egress"
    l4, proto = lay.l4, lay.proto
    addr_at = 26 if egress else 30
    id_at = l4 + (SRC_ID_AT if egress else DST_ID_AT)[proto]
    ck_at = l4 + CSUM_AT[proto]
    may = set(range(addr_at, addr_at + 4)) | {24, 25, id_at, id_at + 1,
                                               ck_at, ck_at + 1}
    bad = []
    stray = [i for i in range(len(before))
             if before[i] != after[i] and i not in may]
    if stray:
        bad.append("bytes outside the translated fields changed at %s"
                   % stray[:16])
    if egress:
        if public_ip is not None and _u32(after, 26) != public_ip:
            bad.append("source %#010x is not the public address %#010x"
                       % (_u32(after, 26), public_ip))
        if port_range is not None and \
                not port_range[0] <= _u16(after, id_at) <= port_range[1]:
            bad.append("port %d outside the block %d..%d"
                       % ((_u16(after, id_at),) + tuple(port_range)))
    # delta invariant, IP header
    hb, ha = (ones_sum(f[14:14 + lay.ihl]) for f in (before, after))
    if not same_sum(hb, ha):
        bad.append("IP header sum moved from %#06x to %#06x" % (hb, ha))
    # delta invariant, L4: addresses (TCP/UDP) plus the L4 bytes present
    if proto == UDP and (_u16(before, ck_at) == 0 or
                         _u16(after, ck_at) == 0):
        if _u16(before, ck_at) != _u16(after, ck_at):
            bad.append("UDP checksum %#06x became %#06x: 'none' and "
                       "'present' must not turn into each other"
                       % (_u16(before, ck_at), _u16(after, ck_at)))
        return bad
    sums = []
    for f in (before, after):
        cover = bytes(f[l4:lay.end])
        if proto != ICMP:
            cover = bytes(f[26:34]) + cover
        sums.append(ones_sum(cover))
    if not same_sum(*sums):
        bad.append("%s sum over addresses and message moved from %#06x to "
                   "%#06x" % (PROTO_NAME[proto], sums[0], sums[1]))
    return bad


# --------------------------------------------------------------- builders
def build_frame(proto, src, dst, *, src_mac, dst_mac=GW_MAC, sport=0,
                dport=0, icmp_type=8, icmp_id=0, payload=b"", options=b"",
                frag=0, l4_csum=None, pad_to=0, padding=None, tcp_flags=0x18,
                ver_ihl=None, truncate=0, ttl=64, ident=0x1234, rng=None):
    """Ethernet + IPv4 [+ options] + TCP/UDP/ICMP, every checksum summed
    from scratch.  frag is the flags+offset word; l4_csum overrides the L4
    checksum field; ver_ihl overrides the first header byte after the
    header checksum was computed for it; truncate cuts bytes off the end
    (the IP total length keeps claiming them)."""
    assert len(options) % 4 == 0 and len(options) <= 40
    if proto == TCP:
        l4 = struct.pack(">HHIIBBHHH", sport, dport, 0x01020304, 0x0A0B0C0D,
                         0x50, tcp_flags, 8192, 0, 0)
    elif proto == UDP:
        l4 = struct.pack(">HHHH", sport, dport, 8 + len(payload), 0)
    else:
        l4 = struct.pack(">BBHHH", icmp_type, 0, 0, icmp_id, 7)
    l4 = bytearray(l4 + payload)
    ihl = 20 + len(options)
    first = ver_ihl if ver_ihl is not None else 0x40 | (ihl // 4)
    ip = bytearray(struct.pack(">BBHHHBBHII", first, 0, ihl + len(l4), ident,
                               frag, ttl, proto, 0, src, dst) + options)
    struct.pack_into(">H", ip, 10, 0xFFFF - ones_sum(ip))
    if l4_csum is None:
        cover = bytes(l4) if proto == ICMP else \
            struct.pack(">IIBBH", src, dst, 0, proto, len(l4)) + bytes(l4)
        l4_csum = 0xFFFF - ones_sum(cover)
        if proto == UDP and l4_csum == 0:
            l4_csum = 0xFFFF
    struct.pack_into(">H", l4, CSUM_AT[proto], l4_csum)
    frame = dst_mac + src_mac + struct.pack(">H", ETH_IP) + bytes(ip) + \
        bytes(l4)
    if pad_to > len(frame):
        k = pad_to - len(frame)
        if padding is None:
            padding = bytes(rng.randrange(1, 256) for _ in range(k)) \
                if rng else b"\xEE" * k
        frame += padding[:k]
    if truncate:
        frame = frame[:-truncate]
    return frame


def expected_egress(frame, public_ip, nat_port):
    """The translation of a whole, well-checksummed datagram, rebuilt the
    sender's way: new source and port in place, both checksums summed
    afresh.  Only for frames `from_scratch_possible` accepts (and UDP
    without a checksum, which stays without)."""
    lay = layout(frame)
    assert not isinstance(lay, str) and lay.whole
    out = bytearray(frame)
    l4, proto = lay.l4, lay.proto
    struct.pack_into(">I", out, 26, public_ip)
    struct.pack_into(">H", out, 24, 0)
    struct.pack_into(">H", out, 24, 0xFFFF - ones_sum(out[14:l4]))
    struct.pack_into(">H", out, l4 + SRC_ID_AT[proto], nat_port)
    ck_at = l4 + CSUM_AT[proto]
    if proto == UDP and _u16(frame, ck_at) == 0:
        return bytes(out)
    struct.pack_into(">H", out, ck_at, 0)
    cover = bytes(out[l4:lay.end])
    if proto != ICMP:
        cover = pseudo_header(out, lay) + cover
    ck = 0xFFFF - ones_sum(cover)
    if proto == UDP and ck == 0:
        ck = 0xFFFF
    struct.pack_into(">H", out, ck_at, ck)
    return bytes(out)


def build_reply(translated, rng, payload_len=None):
    """A fresh datagram from the flow's remote end back to the public
    address and port (or id) of a translated frame."""
    src, dst, proto, sid, did = flow_fields(translated)
    n = rng.choice((0, 1, 2, 3, 17, 18, 31)) if payload_len is None \
        else payload_len
    payload = bytes(rng.randrange(256) for _ in range(n))
    lay = layout(translated)
    icmp_type = {8: 0, 13: 14, 15: 16, 17: 18}.get(translated[lay.l4], 0)
    options = bytes(rng.randrange(256) for _ in range(
        4 * rng.choice((0, 0, 0, 1, 2, 10))))
    return build_frame(proto, dst, src, src_mac=GW_MAC,
                       dst_mac=bytes.fromhex("0200000000fe"),
                       sport=did, dport=sid, icmp_id=sid,
                       icmp_type=icmp_type, payload=payload, tcp_flags=0x10,
                       options=options, pad_to=rng.choice((0, 0, 60)),
                       ident=rng.randrange(0x10000), rng=rng)


# ----------------------------------------------------------------- corpus
#: how the NAT stage must treat a class on egress, for a private source
#: with a NAT context
SCRATCH, DELTA, UNTOUCHED_FWD, UNTOUCHED_PASS = \
    "from-scratch", "delta-only", "untouched-fwd", "untouched-pass"

Sub = namedtuple("Sub", "private_ip mac public_ip port_start port_end")
Entry = namedtuple("Entry", "cls frame sub check")

PUBLIC_DEFAULT = 0xCB007101              # 203.0.113.1


class Corpus:
    """entries[i] = Entry(class name, frame, subscriber, expected check).
    Every frame has a subscriber of its own, so each is the first flow in a
    fresh port block and its NAT port is the block's port_start whatever
    order the frames are processed in."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.entries = []
        self.private = set()
        self.blocks = set()

    def pairs(self):
        return [(e.cls, e.frame) for e in self.entries]

    def classes(self):
        out = {}
        for e in self.entries:
            out.setdefault(e.cls, []).append(e)
        return out

    # -- subscribers
    def new_sub(self, private_ip=None, public_ip=None, block=None):
        """No two subscribers share (public address, block): two flows to
        one destination must not come out with the same public tuple."""
        k = j = len(self.entries)
        if private_ip is None:
            private_ip = 0x0A640000 + (k // 250 << 8) + k % 250 + 1
        assert private_ip not in self.private
        self.private.add(private_ip)
        while True:
            pub = public_ip if public_ip is not None \
                else PUBLIC_DEFAULT + j // 120
            blk = block if block is not None \
                else (2048 + (j % 120) * 512, 2048 + (j % 120) * 512 + 511)
            if (pub, blk[0]) not in self.blocks:
                break
            assert public_ip is None or block is None
            j += 120 if block is not None else 1
        self.blocks.add((pub, blk[0]))
        return Sub(private_ip, (0xAABB00000000 + k).to_bytes(6, "big"),
                   pub, blk[0], blk[1])

    def rand_bytes(self, n):
        return bytes(self.rng.randrange(256) for _ in range(n))

    def add(self, cls, proto, check=SCRATCH, sub=None, **kw):
        sub = sub or self.new_sub()
        rng = self.rng
        kw.setdefault("sport", rng.randrange(1, 0xFFFF))
        kw.setdefault("dport", rng.choice((53, 80, 443, 123, 5060)))
        kw.setdefault("icmp_id", rng.randrange(1, 0xFFFF))
        kw.setdefault("ident", rng.randrange(0x10000))
        kw.setdefault("rng", rng)
        frame = build_frame(proto, sub.private_ip, kw.pop("dst", DST_IP),
                            src_mac=sub.mac, **kw)
        self.entries.append(Entry(cls, frame, sub, check))
        return frame

    def add_landing(self, cls, proto, target, arrive_zero_class=False,
                    solve_input=False, sport=None):
        """Solve the last payload word so that the from-scratch checksum of
        the EXPECTED OUTPUT is `target` (the port is known: the block's
        port_start).  A checksum is the complement of a folded sum that is
        never 0x0000 (the pseudo-header, or the ICMP type, is not zero), so
        0x0000 is reachable and 0xFFFF, its other representation, is not:
        no data sums to it.  An output field of 0xFFFF exists only as UDP's
        replacement for 0x0000.  arrive_zero_class builds the nearest
        thing for the other protocols too: the source port is chosen so
        that old and new address+port sum alike, the checksums of input and
        output are then both zero, and the input carries its own as 0xFFFF
        — an incremental update starts from an all-zero accumulator.
        solve_input makes the INPUT's checksum `target` (zero is carried
        as 0xFFFF) and lets the output land where it will; a target may be
        a function of the subscriber."""
        sub = self.new_sub()
        rng = self.rng
        payload = bytearray(self.rand_bytes(16) + b"\x00\x00")
        if callable(target):
            target = target(sub)
        if sport is None:
            sport = rng.randrange(1024, 0xFFFF)
        if arrive_zero_class:
            new = ones_sum(struct.pack(">IH", sub.public_ip, sub.port_start))
            old = ones_sum(struct.pack(">I", sub.private_ip))
            if proto == ICMP:
                new, old = sub.port_start, 0
            sport = (new - old) % 0xFFFF or 0xFFFF
        out = bytearray(build_frame(
            proto, sub.private_ip, DST_IP, src_mac=sub.mac, sport=sport,
            dport=443, icmp_id=sport, payload=bytes(payload), l4_csum=0))
        lay = layout(out)
        if not solve_input:
            struct.pack_into(">I", out, 26, sub.public_ip)
            struct.pack_into(">H", out, lay.l4 + SRC_ID_AT[proto],
                             sub.port_start)
        cover = bytes(out[lay.l4:lay.end])
        if proto != ICMP:
            cover = pseudo_header(out, lay) + cover
        # checksum field and last word are still zero in `cover`
        payload[16:18] = struct.pack(
            ">H", (0xFFFF - target - ones_sum(cover)) % 0xFFFF)
        kw = dict(l4_csum=0xFFFF) if target == 0 and \
            (arrive_zero_class or solve_input) else {}
        frame = build_frame(proto, sub.private_ip, DST_IP, src_mac=sub.mac,
                            sport=sport, dport=443, icmp_id=sport,
                            payload=bytes(payload), **kw)
        self.entries.append(Entry(cls, frame, sub, SCRATCH))
        return frame


PROTOS = (TCP, UDP, ICMP)


def build_corpus(seed=20260, n_random=96) -> Corpus:
    c = Corpus(seed)
    rng = c.rng
    for p in PROTOS:
        for n in (0, 1, 2, 3, 17, 18, 31):
            c.add("payload_len", p, payload=c.rand_bytes(n))
        for v in (0, 1, 0xFFFF, rng.randrange(2, 0xFFFF)):
            c.add("edge_port", p, sport=v, icmp_id=v,
                  payload=c.rand_bytes(9))
        if p != ICMP:
            for v in (0, 1, 0xFFFF):
                c.add("edge_port", p, dport=v, payload=c.rand_bytes(24))
        c.add("block_1024", p, sub=c.new_sub(block=(1024, 1535)),
              payload=c.rand_bytes(20))
        c.add("block_one_port_65535", p,
              sub=c.new_sub(block=(65535, 65535)), payload=c.rand_bytes(5))
        for pub in (0xFFFF0001, 0x0100FFFF):     # 255.255.0.1, 1.0.255.255
            c.add("public_edge", p, sub=c.new_sub(public_ip=pub),
                  payload=c.rand_bytes(rng.choice((3, 16))))
    for i, p in enumerate(PROTOS):               # 10.0.0.0, 10.1.0.0, ...
        c.add("private_zero_low", p,
              sub=c.new_sub(private_ip=0x0A000000 + (i << 16)),
              payload=c.rand_bytes(14))
    for p in PROTOS:
        c.add_landing("land_0000", p, 0x0000)
        c.add_landing("land_ffff", p, 0x0000, arrive_zero_class=True)
        c.add_landing("land_0001", p, 0x0001)
        c.add_landing("land_fffe", p, 0xFFFE)
        c.add_landing("csum_ffff_in", p, 0x0000, solve_input=True)
    # id 0 and an arriving checksum of port_start - 1: complement of the
    # checksum + complement of the old id + new id = 0x1FFFF, the one sum of
    # three 16-bit terms whose first carry fold (0xFFFF + 1) carries again
    c.add_landing("icmp_double_carry", ICMP, lambda sub: sub.port_start - 1,
                  solve_input=True, sport=0)
    for n in (0, 22, 31):
        c.add("udp_csum_none_in", UDP, l4_csum=0, payload=c.rand_bytes(n))
    # parser branches: the fast parse needs 48 bytes, UDP/ICMP 42, TCP 54
    for p in (UDP, ICMP):
        c.add("short_l4", p, UNTOUCHED_FWD, payload=b"", truncate=1)
        for n in range(42, 50):
            c.add("len_branch", p, payload=c.rand_bytes(n - 42))
    c.add("short_l4", TCP, UNTOUCHED_FWD, truncate=1)
    c.add("len_branch", TCP)
    c.add("len_branch", TCP, payload=c.rand_bytes(1))
    for p in PROTOS:
        for words in (1, 2, 10):                 # ihl 6, 7, 15
            c.add("ip_options", p, options=c.rand_bytes(words * 4),
                  payload=c.rand_bytes(rng.choice((0, 5, 18))))
    c.add("ip_options", TCP, options=c.rand_bytes(40))       # exactly 94
    c.add("short_l4", TCP, UNTOUCHED_FWD, options=c.rand_bytes(40),
          truncate=1)
    for p in PROTOS:
        c.add("eth_padding", p, pad_to=60)
        c.add("eth_padding", p, pad_to=60, payload=c.rand_bytes(3))
        c.add("eth_padding", p, pad_to=64, options=c.rand_bytes(4))
        c.add("bad_l4_csum_in", p, DELTA, l4_csum=rng.randrange(1, 0xFFFF),
              payload=c.rand_bytes(rng.choice((1, 18))))
        c.add("first_fragment", p, DELTA, frag=0x2000,
              l4_csum=rng.randrange(1, 0xFFFF), payload=c.rand_bytes(24))
        for frag in (100, 0x2000 | 100, 1, 0x2000 | 0x1FFF):
            c.add("frag_nonfirst", p, UNTOUCHED_PASS, frag=frag,
                  l4_csum=rng.randrange(0x10000), payload=c.rand_bytes(24))
        for ihl in range(5):
            c.add("bad_ihl", p, UNTOUCHED_FWD, ver_ihl=0x40 | ihl,
                  payload=c.rand_bytes(18))
        for ver in (5, 6):
            c.add("bad_version", p, UNTOUCHED_FWD, ver_ihl=ver << 4 | 5,
                  payload=c.rand_bytes(18))
    for t in (3, 11, 5):
        c.add("icmp_error", ICMP, UNTOUCHED_PASS, icmp_type=t, icmp_id=0,
              payload=c.rand_bytes(28))
        c.add("icmp_error", ICMP, UNTOUCHED_PASS, icmp_type=t,
              icmp_id=rng.randrange(1, 0xFFFF), payload=b"")
    for t in (13, 17):
        c.add("icmp_query", ICMP, icmp_type=t, payload=c.rand_bytes(12))
    for _ in range(n_random):
        p = rng.choice(PROTOS)
        kw = dict(payload=c.rand_bytes(rng.choice((0, 1, 2, 3, 6, 7, 17, 18,
                                                   31, 64, 200))))
        if rng.random() < 0.3:
            kw["options"] = c.rand_bytes(4 * rng.randrange(1, 11))
        if rng.random() < 0.3:
            kw["pad_to"] = rng.choice((60, 64, 128))
        if rng.random() < 0.2:
            kw["sport"] = kw["icmp_id"] = rng.choice((0, 1, 0xFFFF))
        sub = c.new_sub(public_ip=rng.choice(
            (None, 0xFFFF0001, 0x0100FFFF, 0xC6336401)))
        c.add("random", p, sub=sub, **kw)
    return c


def corpus(seed=20260):
    """[(class_name, frame)] — see build_corpus for the subscribers."""
    return build_corpus(seed).pairs()


# ------------------------------------------------- auditing a whole corpus
def ones_sum_header_ok(frame) -> bool:
    lay = layout(frame)
    return not isinstance(lay, str) and \
        ones_sum(frame[14:14 + lay.ihl]) == 0xFFFF


def audit_egress(entry, after) -> list:
    """Problems with `after` as the SNAT stage's output for a corpus entry,
    by the path the entry's class prescribes."""
    before, sub = entry.frame, entry.sub
    if entry.check in (UNTOUCHED_FWD, UNTOUCHED_PASS):
        return untouched(before, after)
    bad = verify_translation(before, after, "egress", sub.public_ip,
                             (sub.port_start, sub.port_end))
    if bad:
        return bad
    lay = layout(before)
    got = _u16(after, lay.l4 + SRC_ID_AT[lay.proto])
    if got != sub.port_start:
        bad.append("port %d is not the fresh block's first, %d"
                   % (got, sub.port_start))
    if entry.check == DELTA:
        if not ones_sum_header_ok(after):
            bad.append("IP header checksum wrong")
        return bad
    assert verify_frame(before) == [], "corpus frame invalid on arrival"
    bad += verify_frame(after)
    if not bad and bytes(after) != expected_egress(before, sub.public_ip,
                                                   sub.port_start):
        bad.append("differs from the datagram rebuilt the sender's way")
    return bad


def audit_ingress(entry, reply, after) -> list:
    """Problems with `after` as the DNAT stage's output for `reply`, a
    datagram sent back to the entry's public address and port."""
    bad = verify_translation(reply, after, "ingress") + verify_frame(after)
    if bad:
        return bad
    _src, dst, _proto, _sid, did = flow_fields(after)
    _s, _d, _p, orig_id, _x = flow_fields(entry.frame)
    if dst != entry.sub.private_ip:
        bad.append("destination %#010x is not the subscriber's" % dst)
    if did != orig_id:
        bad.append("port or id %d is not the original %d" % (did, orig_id))
    return bad


def build_replies(entries, translated, seed=7):
    """One fresh reply per translated entry: [(entry index, reply)]."""
    rng = random.Random(seed)
    return [(i, build_reply(translated[i], rng))
            for i, e in enumerate(entries) if e.check in (SCRATCH, DELTA)]
