"""ICMP errors through NAT44, seen from outside the translator.

RFC 5508 REQ-3/4/5: a NAT must translate an inbound Destination Unreachable,
Time Exceeded or Parameter Problem about one of its flows.  Nothing here
knows how the translator does that.  An error is built the way a router
builds it (`icmp_error`): the IP header of the offending datagram plus `k`
of its bytes, TTL decremented on the way, wrapped in an ICMP message from
the router, every checksum summed from scratch with `wire_oracle.ones_sum`.

The expected output is built the same way and never derived from the input:
for a subscriber's frame `f` and `g = wire_oracle.expected_egress(f, ...)`,
what the NAT sent,

    translate(icmp_error(g -> public address))
        must equal   icmp_error(f -> private address)

byte for byte — the error the subscriber would have got with no NAT on the
path (`same_error`).  Checksum fields compare modulo the two representations
of zero, except a quoted UDP checksum, where 0 means "none" and must stay
what it is.

`build_cases` is the corpus the CPU and the GPU tests share.  Nothing here
imports the golden model or the project's checksum helpers.
"""
import struct
from collections import namedtuple

import wire_oracle as wo

ROUTER_IP = 0xC6336463                   # 198.51.100.99
CORE_MAC = bytes.fromhex("0200000000fe")
ERROR_TYPES = ((3, 0), (3, 1), (3, 3), (3, 4), (3, 13), (11, 0), (11, 1),
               (12, 0))
XLATE, NOMAP, IGNORED = "translated", "unmatched", "ignored"

untouched = wo.untouched


# ------------------------------------------------------------- the builder
def icmp_error(g, to_ip, icmp_type, code, k=None, *, router=ROUTER_IP,
               options=b"", frag=0, ident=0x4242, ttl=250):
    """The error a router sends to `to_ip` about the frame `g`: g's IP
    header and the first `k` bytes behind it (None: the whole datagram).
    options are the OUTER header's; frag its flags+offset word."""
    lay = wo.layout(g)
    assert not isinstance(lay, str), lay
    assert len(options) % 4 == 0
    quoted = bytearray(g[14:lay.l4])
    quoted[8] -= 1                                       # one hop gone
    struct.pack_into(">H", quoted, 10, 0)
    struct.pack_into(">H", quoted, 10, 0xFFFF - wo.ones_sum(quoted))
    data = bytes(g[lay.l4:lay.end])
    quoted += data if k is None else data[:k]
    rest = {(3, 4): 1492, (12, 0): 20 << 24}.get((icmp_type, code), 0)
    icmp = bytearray(struct.pack(">BBHI", icmp_type, code, 0, rest) + quoted)
    struct.pack_into(">H", icmp, 2, 0xFFFF - wo.ones_sum(icmp))
    ihl = 20 + len(options)
    ip = bytearray(struct.pack(">BBHHHBBHII", 0x40 | ihl // 4, 0xC0,
                               ihl + len(icmp), ident, frag, ttl, wo.ICMP, 0,
                               router, to_ip) + options)
    struct.pack_into(">H", ip, 10, 0xFFFF - wo.ones_sum(ip))
    return wo.GW_MAC + CORE_MAC + struct.pack(">H", wo.ETH_IP) + bytes(ip) + \
        bytes(icmp)


def quote_at(err):
    """(outer L4 offset, quoted header offset, quoted L4 offset)."""
    l4 = 14 + (err[14] & 0xF) * 4
    e = l4 + 8
    return l4, e, e + (err[e] & 0xF) * 4


def last_required_byte(err):
    """A frame cut before this length cannot be translated: the quote must
    hold its header and 8 bytes behind it."""
    return quote_at(err)[2] + 8


def refresh_sums(err):
    """Quoted header and outer ICMP checksums summed afresh, after a test
    edited the quote by hand (a router would have sent it consistent)."""
    out = bytearray(err)
    l4, e, q = quote_at(out)
    struct.pack_into(">H", out, e + 10, 0)
    struct.pack_into(">H", out, e + 10, 0xFFFF - wo.ones_sum(out[e:q]))
    struct.pack_into(">H", out, l4 + 2, 0)
    struct.pack_into(">H", out, l4 + 2, 0xFFFF - wo.ones_sum(out[l4:]))
    return bytes(out)


def icmp_residual(err):
    """Ones-complement sum over the whole outer ICMP message, checksum field
    included: 0xFFFF where the checksum is right, and off by as much as the
    checksum is wrong."""
    l4 = quote_at(err)[0]
    return wo.ones_sum(err[l4:])


# -------------------------------------------------------------- the oracle
def checksum_fields(err):
    """{offset: exact?} of every checksum field inside the frame."""
    l4, e, q = quote_at(err)
    out = {24: False, l4 + 2: False, e + 10: False}
    proto = err[e + 9]
    if proto in wo.CSUM_AT and len(err) >= q + wo.CSUM_AT[proto] + 2:
        out[q + wo.CSUM_AT[proto]] = proto == wo.UDP
    return out


def same_error(got, want) -> list:
    """Problems with `got` as the error `want`."""
    got, want = bytes(got), bytes(want)
    if len(got) != len(want):
        return ["length %d, wanted %d" % (len(got), len(want))]
    fields = checksum_fields(want)
    skip = {o + d for o in fields for d in (0, 1)}
    bad = []
    diff = [i for i in range(len(want)) if got[i] != want[i] and i not in skip]
    if diff:
        bad.append("bytes differ at %s" % diff[:16])
    for o, exact in sorted(fields.items()):
        a, b = (struct.unpack_from(">H", x, o)[0] for x in (got, want))
        if a != b and (exact or not wo.same_sum(a, b)):
            bad.append("checksum at %d is %#06x, wanted %#06x" % (o, a, b))
    return bad


def verify_error(err) -> list:
    """What the receiving host rejects a whole (unfragmented, uncut) error
    for: outer header, outer ICMP message, quoted header."""
    bad = wo.verify_frame(err)
    _l4, e, q = quote_at(err)
    s = wo.ones_sum(err[e:q])
    if s != 0xFFFF:
        bad.append("quoted IP header sums to %#06x" % s)
    return bad


# ---------------------------------------------------------------- corpus
#: name; subscriber; frame that opens the flow (None: no flow); the error as
#: it arrives; XLATE / NOMAP / IGNORED; the error wanted back (XLATE only);
#: `stale`: the flow's session is removed before the error arrives
Case = namedtuple("Case", "name sub opener err want expect stale")


class Cases(list):
    def by(self, want):
        return [c for c in self if c.want == want]

    def named(self, prefix):
        return [c for c in self if c.name.startswith(prefix)]

    def openers(self):
        """(subscriber, frame) of every flow to open, each once."""
        seen = {}
        for c in self:
            if c.opener is not None:
                seen.setdefault(c.opener, c.sub)
        return [(sub, f) for f, sub in seen.items()]


def udp_frame_with_sum_zero(c, sub):
    """A subscriber's UDP frame whose checksum computes to zero, so it goes
    out as 0xFFFF: translating the quote back must land on it again."""
    payload = bytearray(c.rand_bytes(10) + b"\x00\x00")
    probe = wo.build_frame(wo.UDP, sub.private_ip, wo.DST_IP, src_mac=sub.mac,
                           sport=40000, dport=53, payload=bytes(payload),
                           l4_csum=0)
    lay = wo.layout(probe)
    s = wo.ones_sum(wo.pseudo_header(probe, lay) + probe[lay.l4:lay.end])
    payload[10:12] = struct.pack(">H", (0xFFFF - s) % 0xFFFF)
    f = wo.build_frame(wo.UDP, sub.private_ip, wo.DST_IP, src_mac=sub.mac,
                       sport=40000, dport=53, payload=bytes(payload))
    assert struct.unpack_from(">H", f, lay.l4 + 6)[0] == 0xFFFF
    assert wo.verify_frame(f) == []
    return f


def build_cases(seed=5508) -> Cases:
    c = wo.Corpus(seed)
    rng = c.rng
    cases = Cases()

    def flow(proto, sub=None, frame=None, **kw):
        """(subscriber, its frame f, what the NAT sends for it g)."""
        sub = sub or c.new_sub()
        c.entries.append(None)               # new_sub counts the entries
        if frame is None:
            kw.setdefault("payload",
                          c.rand_bytes(rng.choice((12, 13, 24, 31))))
            frame = wo.build_frame(
                proto, sub.private_ip, wo.DST_IP, src_mac=sub.mac,
                sport=rng.randrange(1024, 0xFFFF), dport=443,
                icmp_id=rng.randrange(1, 0xFFFF),
                ident=rng.randrange(0x10000), **kw)
        return sub, frame, wo.expected_egress(frame, sub.public_ip,
                                              sub.port_start)

    def positive(name, proto, tc, k, fkw=None, **ekw):
        sub, f, g = flow(proto, **(fkw or {}))
        cases.append(Case(name, sub, f,
                          icmp_error(g, sub.public_ip, *tc, k, **ekw), XLATE,
                          icmp_error(f, sub.private_ip, *tc, k, **ekw),
                          False))

    for proto in wo.PROTOS:
        for tc in ERROR_TYPES:
            for k in (8, 20, None):
                positive("plain", proto, tc, k)
        for k in (8, 20, None):
            positive("quoted_ihl6", proto, (3, 4), k,
                     fkw=dict(options=c.rand_bytes(4)))
            positive("outer_ihl6", proto, (11, 0), k,
                     options=c.rand_bytes(4))
            positive("both_ihl6", proto, (3, 3), k,
                     fkw=dict(options=c.rand_bytes(4)),
                     options=c.rand_bytes(4))
            positive("outer_first_fragment", proto, (3, 1), k, frag=0x2000)
    for k in (8, None):
        positive("udp_csum_none", wo.UDP, (3, 3), k, fkw=dict(l4_csum=0))
    sub = c.new_sub()
    positive("udp_lands_on_zero", wo.UDP, (3, 3), 8,
             fkw=dict(sub=sub, frame=udp_frame_with_sum_zero(c, sub)))
    positive("odd_length_quote", wo.TCP, (3, 4), 19)
    positive("odd_length_quote", wo.UDP, (11, 0), 9)

    def negative(name, want, proto=wo.UDP, tc=(3, 3), k=8, edit=None,
                 open_flow=True, stale=False, to=None, **ekw):
        sub, f, g = flow(proto)
        err = icmp_error(g, sub.public_ip if to is None else to, *tc, k,
                         **ekw)
        if edit:
            out = bytearray(err)
            edit(out, *quote_at(out))
            err = refresh_sums(out)
        cases.append(Case(name, sub, f if open_flow else None, err, want,
                          None, stale))

    def put(off, *values):
        def edit(out, l4, e, q):
            base = {"e": e, "q": q}[off[0]]
            out[base + off[1]:base + off[1] + len(values)] = bytes(values)
        return edit

    for proto in wo.PROTOS:
        for tc in ((4, 0), (5, 1), (5, 0)):      # source quench, redirects
            negative("other_type", IGNORED, proto, tc)
        negative("quoted_src_not_outer_dst", NOMAP, proto,
                 to=0xCB0071FE)                  # somebody else's address
        negative("no_reverse_entry", NOMAP, proto, open_flow=False)
        negative("session_swept", NOMAP, proto, stale=True)
        negative("quoted_fragment", NOMAP, proto, edit=put(("e", 6), 0, 100))
        negative("quoted_version_6", NOMAP, proto, edit=put(("e", 0), 0x65))
        negative("quoted_ihl_4", NOMAP, proto, edit=put(("e", 0), 0x44))
        negative("wrong_remote_address", NOMAP, proto,
                 edit=put(("e", 16), 9, 9, 9, 9))
    for t in (3, 11, 5):
        negative("quoted_icmp_error", NOMAP, wo.ICMP, edit=put(("q", 0), t))
    negative("quoted_other_protocol", NOMAP, edit=put(("e", 9), 47))
    negative("outer_nonfirst_fragment", IGNORED, frag=100)
    negative("outer_nonfirst_fragment", IGNORED, frag=0x2000 | 1)

    # the frame cut at every length from the ICMP header to one byte short
    # of what a translation needs: below 8 bytes of ICMP nobody looks
    for proto, fkw, ekw in ((wo.UDP, {}, {}),
                            (wo.TCP, dict(options=c.rand_bytes(4)),
                             dict(options=c.rand_bytes(4)))):
        sub, f, g = flow(proto, **fkw)
        err = icmp_error(g, sub.public_ip, 3, 4, 8, **ekw)
        l4 = quote_at(err)[0]
        assert last_required_byte(err) == len(err)
        for n in range(l4, len(err)):
            cases.append(Case("cut_%d" % n, sub, f, err[:n],
                              IGNORED if n < l4 + 8 else NOMAP, None, False))
    return cases
