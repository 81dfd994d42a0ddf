"""Exact model of the device token bucket (`qos_tb_check`).

The golden `_tb_check` is the reference's eager bucket: it refills and
moves `last_update` on every packet.  The device bucket is lazy: it
consumes first, refills only when the balance does not cover the packet,
and `last_update` moves only when a refill runs.  The two give the same
verdicts on short trajectories and different state nearly everywhere, so
the device's `tokens` and `last_update` need a model of their own.

This is the sequential meaning of the kernel for one packet per bucket per
launch, where the kernel is deterministic and every field is comparable
exactly.  Plain Python ints throughout: nothing wraps, nothing rounds but
the one floor of the refill.
"""

NS_PER_S = 10**9


def exact_credit(elapsed_ns: int, rate_bps: int) -> int:
    """Bytes earned in elapsed_ns at rate_bps: one floor, no wrap."""
    return elapsed_ns * (rate_bps // 8) // NS_PER_S


class LazyBucket:
    __slots__ = ("rate_bps", "burst", "tokens", "last_update", "refills")

    def __init__(self, rate_bps: int, burst: int, tokens: int,
                 last_update: int):
        self.rate_bps = rate_bps
        self.burst = burst
        self.tokens = tokens
        self.last_update = last_update
        self.refills = 0          # refills that ran (each floors once)

    def _consume(self, pkt_len: int) -> bool:
        if self.tokens >= pkt_len:
            self.tokens -= pkt_len
            return True
        return False

    def offer(self, now_ns: int, pkt_len: int) -> bool:
        if self.rate_bps == 0:
            return True
        if self._consume(pkt_len):
            return True
        if now_ns <= self.last_update:
            # no credit, and the timestamp stays: credit resumes when the
            # clock catches up with it
            return False
        add = exact_credit(now_ns - self.last_update, self.rate_bps)
        self.tokens = min(self.tokens + add, self.burst)
        self.last_update = now_ns
        self.refills += 1
        return self._consume(pkt_len)
