"""Time arithmetic of the token bucket and the NAT sweeper, on the CPU.

`lazy_bucket.LazyBucket` is the exact model the device bucket is compared
with in test_time_arith_gpu.  Here the model itself is pinned: against the
golden eager bucket where the two must agree, against the definition of a
token bucket, and on the three numeric cases a 64-bit implementation gets
wrong.  The golden model's own handling of a clock that steps backwards is
pinned as well, since the device is compared with it.
"""
import math
import random

import pytest

from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import GoldenDataplane, QosBucketRec
from bng_amd.dataplane.launcher import (EIM_TIMEOUT_NS, UDP_TIMEOUT_NS,
                                        GoldenLauncher)
from bng_amd.dataplane.packets import build_ipv4, ip2u32
from lazy_bucket import LazyBucket, exact_credit

NOW = 1_700_000_000 * 10**9
U64 = 1 << 64
RATES = [64_000, 10**9, 10**10]
RATE_IDS = ["64kbps", "1Gbps", "10Gbps"]


def eager(rate, burst, tokens, last):
    """The golden bucket and the dataplane whose clock it reads."""
    dp = GoldenDataplane(now_ns=last)
    return dp, QosBucketRec(rate, burst, tokens, last, 0)


def eager_offer(dp, tb, now, length):
    dp.now_ns = now
    return dp._tb_check(tb, length)


# ------------------------------------------------ model against the golden
@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
def test_model_equals_golden_on_whole_byte_refills_of_an_empty_bucket(rate):
    """Every step earns a whole number of bytes and finds the bucket empty;
    the packets of the step then take exactly what it earned, and one more
    byte is refused.  Eager and lazy must agree on every verdict and on
    (tokens, last_update) after every packet."""
    bps = rate // 8
    # the shortest time that earns whole bytes: `unit` ns earn `per` bytes
    g = math.gcd(bps, 10**9)
    unit, per = 10**9 // g, bps // g
    burst = 4000 * per
    rng = random.Random(rate)
    dp, tb = eager(rate, burst, 0, NOW)
    lazy = LazyBucket(rate, burst, 0, NOW)
    now, passed = NOW, 0
    for step in range(200):
        k = rng.choice([1, 2, 3, 7, 50, 999, 4000, 5000])   # 5000: capped
        now += k * unit
        credit = min(k * per, burst)
        assert exact_credit(now - lazy.last_update, rate) == k * per
        first = rng.randint(1, credit)
        sizes = [first, credit - first, 1] if credit > first else [first, 1]
        for j, length in enumerate(sizes):
            want = j < len(sizes) - 1
            assert lazy.offer(now, length) is want, (step, j)
            assert eager_offer(dp, tb, now, length) is want, (step, j)
            assert (lazy.tokens, lazy.last_update) == \
                (tb.tokens, tb.last_update), (step, j)
            passed += length if want else 0
        assert lazy.tokens == 0
    assert passed > 0


def test_model_and_golden_part_where_the_bucket_is_not_empty():
    """Why the golden cannot pin the device: with tokens in hand the eager
    bucket earns 10.5 ms at a time, floors half a byte away on every packet
    and moves its stamp; the lazy one leaves the stamp until a consume
    fails and then earns the whole interval with one floor."""
    rate, length = 8000, 100                    # 1 byte per ms
    dp, tb = eager(rate, 10**6, 1000, NOW)
    lazy = LazyBucket(rate, 10**6, 1000, NOW)
    now = NOW
    for _ in range(10):
        now += 10_500_000
        assert eager_offer(dp, tb, now, length) and lazy.offer(now, length)
    assert (tb.tokens, tb.last_update) == (100, now)
    assert (lazy.tokens, lazy.last_update) == (0, NOW)
    now += 10_500_000
    assert eager_offer(dp, tb, now, length) and lazy.offer(now, length)
    assert tb.tokens == 10            # 11 floors of 10.5
    assert lazy.tokens == 15          # one floor of 115.5


# -------------------------------------------- model against the definition
@pytest.mark.parametrize("rate,length,step_ns,t_ns", [
    (64_000, 100, 6_250_001, 10 * 10**9),
    (10**9, 1000, 4_001, 10 * 10**6),
    (10**10, 1500, 601, 10**6),
], ids=RATE_IDS)
def test_greedy_source_gets_burst_plus_rate_times_t(rate, length, step_ns,
                                                    t_ns):
    """A source offering twice the rate, one packet per step.  The run ends
    on the first refused packet at or past t_ns, where a refill has just
    run and less than one packet is left: then
        burst + rate/8*T - L - refills <= passed <= burst + rate/8*T
    (the floor loses less than a byte per refill).  The cap never binds
    under a greedy source, so no credit is discarded."""
    bps = rate // 8
    assert length * 10**9 > bps * step_ns       # offered load above the rate
    burst = 10 * length
    b = LazyBucket(rate, burst, burst, NOW)
    now, passed = NOW, 0
    while True:
        now += step_ns
        ok = b.offer(now, length)
        passed += length if ok else 0
        assert 0 <= b.tokens <= burst
        if not ok and now - NOW >= t_ns:
            break
    assert b.last_update == now and b.tokens < length
    earned = bps * (now - NOW) / 10**9
    assert passed <= burst + earned
    assert passed >= burst + earned - length - b.refills
    assert b.refills > 100


# --------------------------------------------------- the three numeric cases
def test_10gbps_idle_14_76_s_wraps_a_64_bit_product():
    elapsed, rate = 14_757_395_259, 10**10
    assert exact_credit(elapsed, rate) == 18_446_744_073
    wrapped = (elapsed * (rate // 8)) % U64
    assert wrapped == 40_448_384 and wrapped // 10**9 == 0
    b = LazyBucket(rate, 0xFFFFFFFF, 0, NOW)
    assert b.offer(NOW + elapsed, 1500)
    assert (b.tokens, b.last_update) == (0xFFFFFFFF - 1500, NOW + elapsed)


def test_101_s_at_64_kbps_earns_808000_bytes_not_the_burst():
    assert exact_credit(101 * 10**9, 64_000) == 808_000
    b = LazyBucket(64_000, 4_000_000, 0, NOW)
    assert b.offer(NOW + 101 * 10**9, 100)
    assert b.tokens == 807_900
    assert not b.offer(NOW + 101 * 10**9, 807_901)


@pytest.mark.parametrize("back", [1, 10 * 10**9])
def test_model_under_a_backward_clock(back):
    drained = LazyBucket(10**9, 10**6, 0, NOW)
    assert not drained.offer(NOW - back, 64)
    assert (drained.tokens, drained.last_update) == (0, NOW)
    full = LazyBucket(10**9, 10**6, 10**6, NOW)
    assert full.offer(NOW - back, 64)
    assert (full.tokens, full.last_update) == (10**6 - 64, NOW)
    # credit resumes where the stamp was left, not where the clock went
    assert drained.offer(NOW + 1000, 125)
    assert (drained.tokens, drained.last_update) == (0, NOW + 1000)


def credit_in_32_bit_digits(elapsed, bytes_per_s, cap):
    """The device's refill credit, step for step in 64-bit words: the
    128-bit product as (hi, lo), then long division by 1e9 in 32-bit
    digits.  Every intermediate must fit 64 bits."""
    D = 10**9
    hi, lo = divmod(elapsed * bytes_per_s, U64)
    if hi >= D:
        return cap
    d1 = (hi << 32) | (lo >> 32)
    assert d1 < U64
    q1 = d1 // D
    d0 = ((d1 - q1 * D) << 32) | (lo & 0xFFFFFFFF)
    assert d0 < U64
    q0 = d0 // D
    return cap if (q1 or q0 > cap) else q0


def test_digitwise_credit_is_exact_over_the_whole_operand_range():
    """elapsed < 2^63, rate < 2^64, any 32-bit cap."""
    rng = random.Random(7)
    edge_e = [0, 1, 999_999_999, 10**9, 14_757_395_259, 100 * 10**9 + 1,
              3600 * 10**9, (1 << 63) - 1]
    edge_r = [0, 7, 8, 64_000, 10**10, 147 * 10**9, 10**11, U64 - 1]
    cases = [(e, r) for e in edge_e for r in edge_r]
    cases += [(rng.getrandbits(rng.randint(1, 63)),
               rng.getrandbits(rng.randint(1, 64))) for _ in range(20000)]
    for e, r in cases:
        for cap in (0, 1500, 0xFFFFFFFF, rng.getrandbits(32)):
            assert credit_in_32_bit_digits(e, r // 8, cap) == \
                min(exact_credit(e, r), cap), (e, r, cap)


# ------------------------------------------ the golden under a backward clock
SUB_IP, PUB_IP, DST = ip2u32("10.1.0.1"), ip2u32("203.0.113.1"), \
    ip2u32("93.184.216.34")


def golden_with_one_flow():
    g = GoldenLauncher()
    g.add_subscriber_nat(SUB_IP, PUB_IP, 1024, 2047, subscriber_id=1)
    f = build_ipv4("aa:bb:cc:00:00:01", "02:00:00:00:00:01", SUB_IP, DST,
                   proto=17, sport=5555, dport=53)
    [(v, _)] = g.process_nat44([f], egress=True, now_ns=NOW)
    assert v == abi.FWD and len(g.dp.nat_sessions) == len(g.dp.eim) == 1
    return g


@pytest.mark.parametrize("back", [1, 10 * 10**9, UDP_TIMEOUT_NS,
                                  EIM_TIMEOUT_NS + 1])
def test_golden_sweep_keeps_what_was_seen_after_now(back):
    g = golden_with_one_flow()
    g.sweep_nat(now_ns=NOW - back)
    assert len(g.dp.nat_sessions) == len(g.dp.nat_reverse) == 1
    assert len(g.dp.eim) == 1
    assert g.nat_get_stats()["sessions_expired"] == 0
    assert g.dp.subnat[SUB_IP].sessions_active == 1
    # and the boundary itself, forwards: kept one ns short, expired on it
    g.sweep_nat(now_ns=NOW + UDP_TIMEOUT_NS - 1)
    assert len(g.dp.nat_sessions) == 1
    g.sweep_nat(now_ns=NOW + UDP_TIMEOUT_NS)
    assert len(g.dp.nat_sessions) == 0 and len(g.dp.eim) == 1
    g.sweep_nat(now_ns=NOW + EIM_TIMEOUT_NS)
    assert len(g.dp.eim) == 0


@pytest.mark.parametrize("back", [1, 10 * 10**9])
def test_golden_tb_check_under_a_backward_clock(back):
    """No debit for negative time and no stamp moved backwards; the verdict
    is the plain consume's."""
    dp, tb = eager(10**9, 10**6, 0, NOW)
    assert not eager_offer(dp, tb, NOW - back, 64)
    assert (tb.tokens, tb.last_update) == (0, NOW)
    dp, tb = eager(10**9, 10**6, 10**6, NOW)
    assert eager_offer(dp, tb, NOW - back, 64)
    assert (tb.tokens, tb.last_update) == (10**6 - 64, NOW)
    # the same bucket under the model
    lazy = LazyBucket(10**9, 10**6, 10**6, NOW)
    assert lazy.offer(NOW - back, 64)
    assert (lazy.tokens, lazy.last_update) == (tb.tokens, tb.last_update)
