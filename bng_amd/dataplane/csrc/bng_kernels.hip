/* bng_kernels.hip — CDNA4 (gfx950) BNG dataplane kernels.
 *
 * MI355X-native re-design of the reference eBPF dataplane:
 *   dhcp_fastpath_kernel  <- bpf/dhcp_fastpath.c:619-813 (XDP)
 *   nat44_egress_kernel   <- bpf/nat44.c:565-802 (TC egress SNAT)
 *   nat44_ingress_kernel  <- bpf/nat44.c:805-948 (TC ingress DNAT)
 *   qos_kernel            <- bpf/qos_ratelimit.c:126-222 (TC token bucket)
 *   antispoof_kernel      <- bpf/antispoof.c:189-293 (TC uRPF)
 *   uplink_pipeline_kernel — fused antispoof+NAT44+QoS+DHCP single pass
 *                            (the per-packet program chain the reference
 *                            runs as four separate TC/XDP hooks)
 *
 * Execution model: one thread per packet, grid-stride, 256-thread blocks
 * (4 waves).  Packet batches are fixed-stride slots in HBM; every lookup
 * table is an open-addressing HBM hash table (bng_abi.h).  Per-packet
 * ktime becomes one host-supplied batch timestamp.  Stats are counted
 * per wave, summed per block in shared memory, and committed with one
 * device-scope atomic per counter per block (bng_device.h).
 *
 * Differential-tested against bng_amd/dataplane/golden.py on random
 * batches (tests/test_kernels_gpu.py).
 */
#include <hip/hip_runtime.h>
#include "bng_abi.h"
#include "bng_params.h"
#include "bng_device.h"
#include "bng_launch.h"

/* ==================================================== table primitives */

typedef __attribute__((address_space(1))) uint64_t gu64_t;

BNG_DEV uint64_t rlx_load64(const void* ptr) {
  return __hip_atomic_load((const uint64_t*)ptr, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}
BNG_DEV void rlx_store64(void* ptr, uint64_t v) {
  __hip_atomic_store((uint64_t*)ptr, v, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

/* Table-probe load: 16 B of a hash-table entry.  BNG_SC1_PROBES=1 issues
 * it as two relaxed agent-scope (sc1) loads — L2-served, bypassing L1 —
 * because random probes have ~0 L1 hit rate and only evict the packet
 * lines the parser needs (same reasoning as the session hit path). */
#ifndef BNG_SC1_PROBES
#define BNG_SC1_PROBES 1
#endif
BNG_DEV uint4 ld_probe16(const void* p) {
#if BNG_SC1_PROBES
  const uint64_t* q = (const uint64_t*)p;
  uint64_t a = rlx_load64(q), b = rlx_load64(q + 1);
  uint4 v;
  v.x = (uint32_t)a; v.y = (uint32_t)(a >> 32);
  v.z = (uint32_t)b; v.w = (uint32_t)(b >> 32);
  return v;
#else
  return *(const uint4*)p;
#endif
}

BNG_DEV uint32_t rlx_load32(const void* ptr) {
  return __hip_atomic_load((const uint32_t*)ptr, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}
BNG_DEV uint32_t rlx_load8(const uint8_t* ptr) {
  return __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

BNG_DEV const bng_sub_entry* sub_lookup(const bng_sub_entry* t, uint32_t mask,
                                        uint64_t key) {
  uint32_t slot = (uint32_t)bng_mix64(key) & mask;
  for (int i = 0; i < BNG_MAX_PROBE; ++i) {
    const bng_sub_entry* e = &t[(slot + i) & mask];
    /* one 16-B vector load covers key+pool_id+allocated_ip (entry is
     * 32-B aligned); most probes end after this single transaction */
    uint4 v = ld_probe16(e);
    uint64_t k = ((uint64_t)v.y << 32) | v.x;
    if (k == key) return e;
    if (k == BNG_KEY_EMPTY) return nullptr;
  }
  return nullptr;
}

/* Merged subscriber-context probe: ONE table walk serves both the NAT
 * port-block and ingress-QoS stages (the reference walks subscriber_nat
 * nat44.c:157-164 AND qos_ingress qos_ratelimit.c:44-50 separately —
 * two random HBM touches per packet; this is one).
 *
 * The hit carries by value everything the per-packet path reads from the
 * entry: the validity flags out of the matching 16-B probe and, for a
 * caller that runs the QoS stage (want_qos), the policy's rate and burst,
 * fetched L1-bypassing right after the key match while the line is being
 * touched anyway.  After the lookup the fused path goes back to the entry
 * only with atomics (tokens, refill claim). */
struct ctx_hit {
  bng_subctx* e;            /* nullptr: no context */
  bool nat_valid, qos_valid;
  uint64_t rate_bps;        /* fetched only with want_qos and qos_valid */
  uint32_t burst_bytes;
};

BNG_DEV ctx_hit ctx_hit_of(bng_subctx* e, uint4 v, bool want_qos) {
  ctx_hit h{e, ((v.w >> 8) & 0xFF) != 0, (v.w & 0xFF) != 0, 0, 0};
  if (want_qos && h.qos_valid) {
    h.rate_bps = rlx_load64(&e->rate_bps);
    h.burst_bytes = rlx_load32(&e->burst_bytes);
  }
  return h;
}

BNG_DEV ctx_hit subctx_lookup_hint(bng_subctx* t, uint32_t mask, uint32_t ip,
                                   uint32_t slot, uint4 first,
                                   bool want_qos) {
  const ctx_hit none{nullptr, false, false, 0, 0};
  if (first.x == ip) return ctx_hit_of(&t[slot], first, want_qos);
  if (first.x == 0) return none;
  for (int i = 1; i < BNG_MAX_PROBE; ++i) {
    bng_subctx* e = &t[(slot + i) & mask];
    uint4 v = ld_probe16(e);
    if (v.x == ip) return ctx_hit_of(e, v, want_qos);
    if (v.x == 0) return none;
  }
  return none;
}

BNG_DEV ctx_hit subctx_lookup(bng_subctx* t, uint32_t mask, uint32_t ip,
                              bool want_qos) {
  if (ip == 0) return ctx_hit{nullptr, false, false, 0, 0};
  uint32_t slot = (uint32_t)bng_mix64(ip) & mask;
  /* key + pub_ip + ports + valid flags */
  return subctx_lookup_hint(t, mask, ip, slot, ld_probe16(&t[slot]),
                            want_qos);
}

BNG_DEV bng_qos_bucket* qos_lookup(bng_qos_bucket* t, uint32_t mask,
                                   uint32_t ip, uint64_t* rate_out) {
  if (ip == 0) return nullptr;
  uint32_t slot = (uint32_t)bng_mix64(ip) & mask;
  for (int i = 0; i < BNG_MAX_PROBE; ++i) {
    bng_qos_bucket* e = &t[(slot + i) & mask];
    uint4 v = ld_probe16(e);    /* key_ip+valid+prio | rate in 16B */
    if (v.x == ip && (v.y & 0xFF)) {
      *rate_out = ((uint64_t)v.w << 32) | v.z;
      return e;
    }
    if (v.x == 0) return nullptr;
  }
  return nullptr;
}

/* A binding as the antispoof stage sees it: the matching 16-B probe holds
 * key_mac, ipv4_addr, ipv4_valid, ipv6_valid and mode, so the IPv4 check
 * takes them by value; only the IPv6 compare goes back to the entry. */
struct bind_hit {
  const bng_binding_entry* e;   /* nullptr: unknown MAC */
  uint32_t ipv4_addr;
  bool ipv4_valid, ipv6_valid;
  uint8_t mode;
};

BNG_DEV bind_hit bind_hit_of(const bng_binding_entry* e, uint4 v) {
  return bind_hit{e, v.z, (v.w & 0xFF) != 0, ((v.w >> 8) & 0xFF) != 0,
                  (uint8_t)(v.w >> 16)};
}

BNG_DEV bind_hit binding_lookup_hint(const bng_binding_entry* t,
                                     uint32_t mask, uint64_t mac,
                                     uint32_t slot, uint4 first) {
  const bind_hit none{nullptr, 0, false, false, 0};
  uint64_t k = ((uint64_t)first.y << 32) | first.x;
  if (k == mac) return bind_hit_of(&t[slot], first);
  if (k == BNG_KEY_EMPTY) return none;
  for (int i = 1; i < BNG_MAX_PROBE; ++i) {
    const bng_binding_entry* e = &t[(slot + i) & mask];
    uint4 v = ld_probe16(e);
    k = ((uint64_t)v.y << 32) | v.x;
    if (k == mac) return bind_hit_of(e, v);
    if (k == BNG_KEY_EMPTY) return none;
  }
  return none;
}

BNG_DEV bind_hit binding_lookup(const bng_binding_entry* t, uint32_t mask,
                                uint64_t mac) {
  if (mac == 0) return bind_hit{nullptr, 0, false, false, 0};
  uint32_t slot = (uint32_t)bng_mix64(mac) & mask;
  /* key + ipv4 + flags in one load */
  return binding_lookup_hint(t, mask, mac, slot, ld_probe16(&t[slot]));
}

/* find-or-claim for device-created entries (sessions / EIM / reverse).
 * Returns the entry, with `claimed` set when this thread won the slot; on
 * a sig match (`found`) the caller must bng_wait_ready() before trusting
 * fields.
 * Tombstoned slots (sweep-expired sessions) are RECLAIMED: the probe
 * remembers the first tombstone and claims it once the full chain
 * rules out an existing entry — without this, long-uptime churn fills
 * the chain with tombstones (the reference gets reuse for free from
 * BPF LRU maps). */
/* Post-claim duplicate check (round-1 advisor finding): if a chain slot
 * is tombstoned concurrently (in-batch port-exhaustion release), one
 * lane can reclaim that earlier tombstone while another lane of the
 * SAME flow claims a later slot — leaking a duplicate session + NAT
 * port until sweep.  After winning a claim CAS, rescan the chain for a
 * concurrent same-sig insert and keep only the EARLIEST-position claim:
 * the later claimant re-tombstones its slot and adopts the earlier one.
 * The positional tie-break is what makes this safe for lockstep lanes —
 * a symmetric release-on-any-hit rule would make two same-wave lanes
 * release each other every retry.  Residual window: a later claimant
 * whose rescan completed before our CAS landed keeps a shadowed
 * duplicate; that reverts to the pre-fix behavior (sweep reclaims it,
 * EIM collision check keeps the port safe) in a window now measured in
 * the tens of nanoseconds instead of the whole create race. */
/* What a find-or-claim returns, by value: out-parameters took their
 * address at every call site and lived in scratch memory. */
template <typename E>
struct claim_res {
  E* e;                     /* nullptr: chain full of other keys */
  bool claimed, found;
};

template <typename E>
BNG_DEV claim_res<E> claim_dedup(E* t, uint32_t mask, uint64_t sig,
                                 uint32_t slot, int my_pos) {
  for (int i = 0; i < BNG_MAX_PROBE; ++i) {
    if (i == my_pos) continue;
    E* e = &t[(slot + i) & mask];
    uint64_t k = __hip_atomic_load(&e->sig, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    if (k == sig && i < my_pos) {
      /* earlier claim wins: release ours, adopt theirs (caller does
       * bng_wait_ready before trusting fields) */
      __hip_atomic_store(&t[(slot + my_pos) & mask].sig,
                         BNG_KEY_TOMBSTONE, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      return claim_res<E>{e, false, true};
    }
    if (k == BNG_KEY_EMPTY) break;
  }
  return claim_res<E>{&t[(slot + my_pos) & mask], true, false};
}

template <typename E>
BNG_DEV claim_res<E> sig_find_or_claim(E* t, uint32_t mask, uint64_t sig) {
  const claim_res<E> full{nullptr, false, false};
  uint32_t slot = (uint32_t)sig & mask;
  /* pass 1 — pure hit scan, identical cost to the pre-reclamation hot
   * path (hits dominate: established flows) */
  for (int i = 0; i < BNG_MAX_PROBE; ++i) {
    E* e = &t[(slot + i) & mask];
    uint64_t k = __hip_atomic_load(&e->sig, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    if (k == sig) return claim_res<E>{e, false, true};
    if (k == BNG_KEY_EMPTY) break;
  }
  /* pass 2 — claim scan (session-create path only) */
  for (int attempt = 0; attempt < 4; ++attempt) {
    int first_tomb = -1, first_tomb_pos = -1;
    for (int i = 0; i < BNG_MAX_PROBE; ++i) {
      E* e = &t[(slot + i) & mask];
      uint64_t k = __hip_atomic_load(&e->sig, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
      if (k == sig) return claim_res<E>{e, false, true};
      if (k == BNG_KEY_TOMBSTONE) {
        if (first_tomb < 0) {
          first_tomb = (int)((slot + i) & mask);
          first_tomb_pos = i;
        }
        continue;
      }
      if (k == BNG_KEY_EMPTY) {
        E* d = first_tomb >= 0 ? &t[first_tomb] : e;
        int d_pos = first_tomb >= 0 ? first_tomb_pos : i;
        uint64_t want = first_tomb >= 0 ? BNG_KEY_TOMBSTONE
                                        : BNG_KEY_EMPTY;
        if (__hip_atomic_compare_exchange_strong(
                &d->sig, &want, sig, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                __HIP_MEMORY_SCOPE_AGENT)) {
          return claim_dedup(t, mask, sig, slot, d_pos);
        }
        if (want == sig) return claim_res<E>{d, false, true};
        /* lost the slot to a DIFFERENT key: keep probing.  If it was
         * the remembered tombstone, forget it and retry this empty
         * slot; if it was the empty slot itself, scan past it. */
        if (first_tomb >= 0) { first_tomb = -1; first_tomb_pos = -1; --i; }
        continue;
      }
    }
    if (first_tomb < 0)
      return full;               /* chain genuinely full of other keys */
    /* chain full but reclaimable: take the tombstone directly */
    E* d = &t[first_tomb];
    uint64_t want = BNG_KEY_TOMBSTONE;
    if (__hip_atomic_compare_exchange_strong(
            &d->sig, &want, sig, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_AGENT)) {
      return claim_dedup(t, mask, sig, slot, first_tomb_pos);
    }
    if (want == sig) return claim_res<E>{d, false, true};
    /* raced: rescan */
  }
  return full;
}

template <typename E>
BNG_DEV E* sig_lookup(E* t, uint32_t mask, uint64_t sig) {
  uint32_t slot = (uint32_t)sig & mask;
  for (int i = 0; i < BNG_MAX_PROBE; ++i) {
    E* e = &t[(slot + i) & mask];
    uint64_t k = __hip_atomic_load(&e->sig, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    if (k == sig) return e;
    if (k == BNG_KEY_EMPTY) return nullptr;
  }
  return nullptr;
}

/* Probes of the host CRUD kernels (one thread per batch record).
 *
 * Key accesses: key loads, the claim CAS and tombstone stores are relaxed,
 * agent scope.  Value fields are plain stores after the claim; there is no
 * `ready` flag — stream order publishes the entry to the packet kernels.
 *
 * Batch contract: a batch must not name the same key twice.  On a lost CAS
 * the thread forgets its remembered tombstone and goes on with the NEXT
 * slot; it does not re-read the lost one, so a duplicate key in one batch
 * could land in two slots.
 *
 * 64-bit-key tables (K = &E::<key field>; 0 empty, ~0 tombstone): an upsert
 * takes the first tombstone of its chain, but only once an empty slot
 * proves the key absent.  Known limitation: a chain with tombstones but NO
 * empty slot within BNG_MAX_PROBE reports full (nullptr) although it is
 * reclaimable; sig_find_or_claim handles that case, and this is the one
 * place to fix it. */
template <auto K, typename E>
BNG_DEV E* key_upsert_slot(E* t, uint32_t mask, uint64_t key) {
  uint32_t slot = (uint32_t)bng_mix64(key) & mask;
  E* tomb = nullptr;
  for (int i = 0; i < BNG_MAX_PROBE; ++i) {
    E* e = &t[(slot + i) & mask];
    uint64_t cur = rlx_load64(&(e->*K));
    if (cur == key) return e;
    if (cur == BNG_KEY_TOMBSTONE && !tomb) tomb = e;
    if (cur == BNG_KEY_EMPTY) {
      E* d = tomb ? tomb : e;
      uint64_t expect = tomb ? BNG_KEY_TOMBSTONE : BNG_KEY_EMPTY;
      if (__hip_atomic_compare_exchange_strong(
              &(d->*K), &expect, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
              __HIP_MEMORY_SCOPE_AGENT))
        return d;
      tomb = nullptr;   /* raced with another upsert of this batch */
    }
  }
  return nullptr;       /* probe bound exceeded: table too full */
}

/* Find for the deletes (the caller stores the tombstone): walks past
 * tombstones, stops at empty; an absent key is nullptr. */
template <auto K, typename E>
BNG_DEV E* key_find(E* t, uint32_t mask, uint64_t key) {
  uint32_t slot = (uint32_t)bng_mix64(key) & mask;
  for (int i = 0; i < BNG_MAX_PROBE; ++i) {
    E* e = &t[(slot + i) & mask];
    uint64_t cur = rlx_load64(&(e->*K));
    if (cur == key) return e;
    if (cur == BNG_KEY_EMPTY) return nullptr;
  }
  return nullptr;
}

/* 32-bit key_ip tables (bng_subctx, bng_qos_bucket; 0 empty, no
 * tombstones).  nullptr with *full unset: the key is absent and
 * claim_if_absent was false. */
template <typename E>
BNG_DEV E* ipkey_upsert_slot(E* t, uint32_t mask, uint32_t ip,
                             bool claim_if_absent, bool* full) {
  *full = false;
  uint32_t slot = (uint32_t)bng_mix64(ip) & mask;
  for (int i = 0; i < BNG_MAX_PROBE; ++i) {
    E* e = &t[(slot + i) & mask];
    uint32_t cur = __hip_atomic_load(&e->key_ip, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
    if (cur == ip) return e;
    if (cur == 0) {
      if (!claim_if_absent) return nullptr;
      if (__hip_atomic_compare_exchange_strong(
              &e->key_ip, &cur, ip, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
              __HIP_MEMORY_SCOPE_AGENT))
        return e;
    }
  }
  *full = true;
  return nullptr;
}

BNG_DEV bool tuple_eq(const bng_nat_tuple& a, const bng_nat_tuple& b) {
  return a.src_ip == b.src_ip && a.dst_ip == b.dst_ip &&
         a.src_port == b.src_port && a.dst_port == b.dst_port &&
         a.protocol == b.protocol;
}

/* ===================================================== parsed context */

struct pktctx {
  uint8_t* p;        /* slot base */
  int len;
  int ip_off;        /* -1 if not IPv4 */
  int l4_off;
  uint8_t proto;
  uint32_t saddr, daddr;      /* big-endian byte order, as host ints */
  uint16_t sport, dport;      /* host ints of the BE fields */
  uint16_t icmp_id;
  uint8_t tcp_flags;
  /* vlan */
  int vlan_offset;
  uint16_t s_tag, c_tag;
  bool tagged;
  /* ports or ICMP id parsed.  Never set for a non-first fragment (no L4
   * header in the frame) or an ICMP message that is not a query (no id
   * field): their L4 bytes are neither read nor written */
  bool l4_ok;
  /* register window: bswapped words of bytes 0..47 when the fast parse
   * ran (untagged ihl=5).  TA (vector-memory address) occupancy is the
   * measured kernel bound — header rewrites happen on these registers
   * and flush as two dwordx4 stores instead of ~10 divergent byte ops */
  uint32_t W[12];
  bool regs;
};

/* constant-offset register accessors (offsets fold at compile time).
 * The w_* forms work on any window of bswapped words, `o` counted from
 * the window's first byte; the rg_* forms are the packet's bytes 0..47. */
template <int N> BNG_DEV uint32_t w_ld8(const uint32_t (&W)[N], int o) {
  return (W[o >> 2] >> (24 - 8 * (o & 3))) & 0xFFu;
}
template <int N> BNG_DEV uint32_t w_ld16(const uint32_t (&W)[N], int o) {
  return (w_ld8(W, o) << 8) | w_ld8(W, o + 1);
}
template <int N> BNG_DEV uint32_t w_ld32(const uint32_t (&W)[N], int o) {
  return (w_ld16(W, o) << 16) | w_ld16(W, o + 2);
}
template <int N> BNG_DEV void w_st8(uint32_t (&W)[N], int o, uint32_t v) {
  int i = o >> 2, sh = 24 - 8 * (o & 3);
  W[i] = (W[i] & ~(0xFFu << sh)) | ((v & 0xFFu) << sh);
}
template <int N> BNG_DEV void w_st16(uint32_t (&W)[N], int o, uint32_t v) {
  w_st8(W, o, v >> 8); w_st8(W, o + 1, v);
}
template <int N> BNG_DEV void w_st32(uint32_t (&W)[N], int o, uint32_t v) {
  w_st16(W, o, v >> 16); w_st16(W, o + 2, v);
}
/* words 4k..4k+3 of a window as the 16 B they came from */
template <int N> BNG_DEV uint4 w_chunk(const uint32_t (&W)[N], int k) {
  return make_uint4(__builtin_bswap32(W[4 * k]),
                    __builtin_bswap32(W[4 * k + 1]),
                    __builtin_bswap32(W[4 * k + 2]),
                    __builtin_bswap32(W[4 * k + 3]));
}
#define RG_B(c, o) (((c).W[(o) >> 2] >> (24 - 8 * ((o) & 3))) & 0xFFu)
BNG_DEV uint16_t rg_ld16(const pktctx& c, int o) {
  return (uint16_t)((RG_B(c, o) << 8) | RG_B(c, o + 1));
}
BNG_DEV void rg_st8(pktctx& c, int o, uint32_t v) { w_st8(c.W, o, v); }
BNG_DEV void rg_st16(pktctx& c, int o, uint32_t v) { w_st16(c.W, o, v); }
BNG_DEV void rg_st32(pktctx& c, int o, uint32_t v) { w_st32(c.W, o, v); }
BNG_DEV void rg_flush16_47(pktctx& c) {
  uint4* q = (uint4*)c.p;
  q[1] = make_uint4(__builtin_bswap32(c.W[4]), __builtin_bswap32(c.W[5]),
                    __builtin_bswap32(c.W[6]), __builtin_bswap32(c.W[7]));
  q[2] = make_uint4(__builtin_bswap32(c.W[8]), __builtin_bswap32(c.W[9]),
                    __builtin_bswap32(c.W[10]),
                    __builtin_bswap32(c.W[11]));
}

/* ICMP types with an id at bytes 4..5: echo, timestamp, information and
 * address-mask requests and replies (0, 8, 13..18) */
BNG_DEV bool icmp_is_query(uint32_t type) {
  return type <= 18 && ((0x7E101u >> type) & 1u);
}

/* Bytes 0..47 of the frame into the register window, as one burst of
 * three plain 16-B loads.  The L1-bypassing form (8-B agent-scope pairs)
 * was measured and left out: in the fused kernel it fetched no fewer lines
 * from memory, cost 5 M more L2 requests per 1M packets and slowed the
 * stand-alone kernels (profiles/EA_BUDGET.md).  False (nothing loaded) for
 * a short frame or a row that is not 16-B aligned. */
BNG_DEV bool pkt_window_load(pktctx& c, const uint8_t* p, int len) {
  if (len < 48 || ((uintptr_t)p & 15)) return false;
  /* no alias pointer to c.W: an escaping pointer would force the
   * register window into scratch memory */
  #pragma unroll
  for (int i = 0; i < 3; ++i) {
    uint4 v = ((const uint4*)p)[i];
    c.W[i * 4 + 0] = __builtin_bswap32(v.x);
    c.W[i * 4 + 1] = __builtin_bswap32(v.y);
    c.W[i * 4 + 2] = __builtin_bswap32(v.z);
    c.W[i * 4 + 3] = __builtin_bswap32(v.w);
  }
  return true;
}

/* Vectorized parse fast path on a loaded window: untagged IPv4 with ihl=5
 * (the 64B-mix hot case).  Three 16-B loads replace ~30 dependent byte
 * loads; fields are extracted from registers with constant shifts.
 * Returns false to fall back to the general byte parser (VLAN, options). */
BNG_DEV bool parse_pkt_window(pktctx& c, uint8_t* p, int len) {
  #define BNG_B(o) ((c.W[(o) >> 2] >> (24 - 8 * ((o) & 3))) & 0xFFu)
  #define BNG_H(o) ((BNG_B(o) << 8) | BNG_B((o) + 1))
  uint32_t ethertype = BNG_H(12);
  if (ethertype != 0x0800) return false;        /* VLAN etc: slow path */
  if (BNG_B(14) != 0x45) return false;          /* options/ihl!=5 */
  c.p = p; c.len = len; c.vlan_offset = 0; c.s_tag = c.c_tag = 0;
  c.tagged = false; c.l4_ok = false;
  c.regs = true;
  c.ip_off = 14;
  c.proto = (uint8_t)BNG_B(23);
  c.saddr = (BNG_H(26) << 16) | BNG_H(28);
  c.daddr = (BNG_H(30) << 16) | BNG_H(32);
  c.l4_off = 34;
  if (BNG_H(20) & 0x1FFFu) {
    /* non-first fragment: no L4 header */
  } else if (c.proto == 6 && len >= 54) {
    c.sport = (uint16_t)BNG_H(34);
    c.dport = (uint16_t)BNG_H(36);
    c.tcp_flags = (uint8_t)BNG_B(47);
    c.l4_ok = true;
  } else if (c.proto == 17 && len >= 42) {
    c.sport = (uint16_t)BNG_H(34);
    c.dport = (uint16_t)BNG_H(36);
    c.l4_ok = true;
  } else if (c.proto == 1 && len >= 42) {
    if (icmp_is_query(BNG_B(34))) {
      c.icmp_id = (uint16_t)BNG_H(38);
      c.l4_ok = true;
    }
  }
  #undef BNG_B
  #undef BNG_H
  return true;
}

/* Parse Ethernet [+VLAN/QinQ] + IPv4 + L4 ports.  NAT/QoS/antispoof paths
 * in the reference parse untagged frames only (nat44.c:573-581); the DHCP
 * path handles tags (dhcp_fastpath.c:352-428).  want_vlan selects. */
BNG_DEV bool parse_pkt_slow(pktctx& c, uint8_t* p, int len, bool want_vlan) {
  c.p = p; c.len = len; c.ip_off = -1; c.vlan_offset = 0;
  c.s_tag = c.c_tag = 0; c.tagged = false; c.l4_ok = false;
  c.regs = false;
  if (len < 14) return false;
  uint16_t proto = ld_u16be(p + 12);
  int off = 14;
  if (want_vlan && (proto == 0x8100 || proto == 0x88A8)) {
    if (len < off + 4) return false;
    c.tagged = true;
    c.s_tag = ld_u16be(p + off) & 0xFFF;
    proto = ld_u16be(p + off + 2);
    off += 4; c.vlan_offset = 4;
    if (proto == 0x8100) {
      if (len < off + 4) return false;
      c.c_tag = ld_u16be(p + off) & 0xFFF;
      proto = ld_u16be(p + off + 2);
      off += 4; c.vlan_offset = 8;
    }
  }
  if (proto != 0x0800 || len < off + 20) return false;
  /* not version 4, or a header shorter than the fixed 20 bytes: not an
   * IPv4 packet, whatever the ethertype says */
  uint8_t vihl = p[off];
  if ((vihl >> 4) != 4 || (vihl & 0xF) < 5) return false;
  c.ip_off = off;
  c.proto = p[off + 9];
  c.saddr = ld_u32be(p + off + 12);
  c.daddr = ld_u32be(p + off + 16);
  int ihl = (vihl & 0xF) * 4;
  c.l4_off = off + ihl;
  if (ld_u16be(p + off + 6) & 0x1FFF) {
    /* non-first fragment: no L4 header */
  } else if (c.proto == 6 && len >= c.l4_off + 20) {
    c.sport = ld_u16be(p + c.l4_off);
    c.dport = ld_u16be(p + c.l4_off + 2);
    c.tcp_flags = p[c.l4_off + 13];
    c.l4_ok = true;
  } else if (c.proto == 17 && len >= c.l4_off + 8) {
    c.sport = ld_u16be(p + c.l4_off);
    c.dport = ld_u16be(p + c.l4_off + 2);
    c.l4_ok = true;
  } else if (c.proto == 1 && len >= c.l4_off + 8) {
    if (icmp_is_query(p[c.l4_off])) {
      c.icmp_id = ld_u16be(p + c.l4_off + 4);
      c.l4_ok = true;
    }
  }
  return true;
}

BNG_DEV bool parse_pkt(pktctx& c, uint8_t* p, int len, bool want_vlan) {
  if (pkt_window_load(c, p, len) && parse_pkt_window(c, p, len)) return true;
  return parse_pkt_slow(c, p, len, want_vlan);
}

/* ================================================== DHCP fast path K1 */

struct dhcp_tables {
  const bng_sub_entry* subs; uint32_t sub_mask;
  const bng_ip_pool* pools;  uint32_t n_pools;
  const bng_server_config* cfg;
  unsigned long long* stats;
  uint64_t now_sec;
};

/* stats flags gathered per packet, ballot-aggregated by the caller */
struct dhcp_flags {
  bool vlan, total, hit, miss, expired, error, o82, bcast, ucast;
  BNG_DEV void clear() {
    vlan = total = hit = miss = expired = error = o82 = bcast = ucast = false;
  }
};

/* Scan DHCP options for msg-type (53) and option-82 circuit-id.  Full TLV
 * scan — the GPU has no verifier, so we upgrade the reference's
 * fixed-offset workaround (dhcp_fastpath.c:216-323) while keeping its
 * bounds (64 options / 312 bytes, maps.h:19-22). */
BNG_DEV void scan_dhcp_options(const uint8_t* p, int opt_off, int end,
                               uint8_t* msg_type, const uint8_t** cid,
                               int* cid_len) {
  *msg_type = 0; *cid = nullptr; *cid_len = 0;
  int i = opt_off;
  int limit = min(end, opt_off + 312);
  for (int iters = 0; iters < 64 && i < limit; ++iters) {
    uint8_t code = p[i];
    if (code == 0) { ++i; continue; }
    if (code == 255) break;
    if (i + 1 >= limit) break;
    uint8_t ln = p[i + 1];
    if (i + 2 + ln > limit) break;
    if (code == 53 && ln == 1) *msg_type = p[i + 2];
    else if (code == 82) {
      int j = i + 2, sub_end = i + 2 + ln;
      while (j + 2 <= sub_end) {
        uint8_t sc = p[j], sl = p[j + 1];
        if (j + 2 + sl > sub_end) break;
        if (sc == 1 && sl > 0 && sl <= 32) { *cid = p + j + 2; *cid_len = sl; }
        j += 2 + sl;
      }
    }
    i += 2 + ln;
  }
}

/* ---- wide reply builder.  When the fast parse ran (untagged, ihl 5,
 * 16-B aligned row) every offset of the reply is a constant: Ethernet 0,
 * IP 14, UDP 34, BOOTP 42 (op 42, hops 45, flags 52, ciaddr 54, yiaddr 58,
 * siaddr 62, giaddr 66, chaddr 70, sname 86, file 150, cookie 278,
 * options 282).  The reply is then composed in registers and leaves as
 * 16-B stores instead of ~110 byte/short/dword stores per packet:
 *   bytes   0..47   the parse's register window (headers, op, hops)
 *   bytes  48..95   loaded before the lookup (it also feeds chaddr,
 *                   giaddr, flags and ciaddr), patched, stored back
 *   bytes  96..271  zeros (sname/file)
 *   bytes 272..     tail of `file`, the cookie, the options
 * It writes exactly the bytes the byte-wise builder writes, no byte
 * more: the last, partial 16 B go out as exact-width stores.  The row
 * must hold the longest reply. */
enum {
  BNG_DHCP_OPT_OFF = 282,          /* untagged ihl-5 frame */
  BNG_DHCP_MAX_OPTS = 50,          /* with two DNS servers */
  BNG_DHCP_WIDE_MIN_STRIDE = 336   /* 272 + 4 chunks */
};

struct dhcp_reply {                /* what both builders put on the wire */
  uint32_t yiaddr, server_ip;
  uint8_t reply_type;
};

BNG_DEV uint32_t pool_netmask(const bng_ip_pool& pool) {
  return (pool.prefix_len == 0) ? 0
      : (pool.prefix_len >= 32) ? 0xFFFFFFFFu
      : (0xFFFFFFFFu << (32 - pool.prefix_len));
}

/* options 53/54/51/1/3/[6]/58/59/255 into the window O (bytes 272..335 of
 * the row), NDNS servers in option 6; then the stores from byte 272 on */
template <int NDNS>
BNG_DEV void dhcp_wide_options(uint8_t* p, const dhcp_reply& R,
                               const bng_ip_pool& pool) {
  uint32_t O[16];
  #pragma unroll
  for (int i = 0; i < 16; ++i) O[i] = 0;
  int o = 6;                       /* 272..277: end of `file`, zero */
  w_st32(O, o, 0x63825363u); o += 4;
  w_st8(O, o, 53); w_st8(O, o + 1, 1); w_st8(O, o + 2, R.reply_type); o += 3;
  w_st8(O, o, 54); w_st8(O, o + 1, 4); w_st32(O, o + 2, R.server_ip); o += 6;
  w_st8(O, o, 51); w_st8(O, o + 1, 4); w_st32(O, o + 2, pool.lease_time);
  o += 6;
  w_st8(O, o, 1); w_st8(O, o + 1, 4); w_st32(O, o + 2, pool_netmask(pool));
  o += 6;
  w_st8(O, o, 3); w_st8(O, o + 1, 4); w_st32(O, o + 2, pool.gateway); o += 6;
  if (NDNS) {
    w_st8(O, o, 6); w_st8(O, o + 1, 4 * NDNS);
    w_st32(O, o + 2, pool.dns_primary);
    if (NDNS == 2) w_st32(O, o + 6, pool.dns_secondary);
    o += 2 + 4 * NDNS;
  }
  w_st8(O, o, 58); w_st8(O, o + 1, 4); w_st32(O, o + 2, pool.lease_time / 2);
  o += 6;
  w_st8(O, o, 59); w_st8(O, o + 1, 4);
  w_st32(O, o + 2, (pool.lease_time * 7) / 8); o += 6;
  w_st8(O, o, 255); o += 1;
  /* o = 50 / 56 / 60: three whole chunks, then 2 / 8 / 12 bytes */
  uint4* q = (uint4*)(p + 272);
  q[0] = w_chunk(O, 0); q[1] = w_chunk(O, 1); q[2] = w_chunk(O, 2);
  uint4 t = w_chunk(O, 3);
  if (NDNS == 0) {
    *(uint16_t*)(p + 320) = (uint16_t)t.x;
  } else {
    *(uint2*)(p + 320) = make_uint2(t.x, t.y);
    if (NDNS == 2) *(uint32_t*)(p + 328) = t.z;
  }
}

/* c.W holds bytes 0..47 and X bytes 48..95 of the request; returns the
 * frame length of the reply and sets *bcast when it goes to the broadcast
 * MAC */
BNG_DEV int dhcp_reply_wide(pktctx& c, uint32_t (&X)[12],
                            const dhcp_reply& R, const bng_ip_pool& pool,
                            const bng_server_config& cfg, bool& bcast) {
  bcast = false;
  uint8_t* p = c.p;
  const int ndns = pool.dns_primary ? (pool.dns_secondary ? 2 : 1) : 0;
  const int w = 40 + (ndns ? 2 + 4 * ndns : 0);
  uint32_t giaddr = w_ld32(X, 66 - 48);
  uint32_t smac_hi = ((uint32_t)cfg.server_mac[0] << 8) | cfg.server_mac[1];
  uint32_t smac_lo = ((uint32_t)cfg.server_mac[2] << 24) |
                     ((uint32_t)cfg.server_mac[3] << 16) |
                     ((uint32_t)cfg.server_mac[4] << 8) | cfg.server_mac[5];
  uint32_t dst_ip, dport;
  if (giaddr != 0) {   /* relayed: unicast to relay agent (ref :726-743) */
    uint32_t hi = rg_ld16(c, 6);
    uint32_t lo = ((uint32_t)rg_ld16(c, 8) << 16) | rg_ld16(c, 10);
    rg_st16(c, 0, hi); rg_st32(c, 2, lo);
    dst_ip = giaddr; dport = 67;
  } else {
    uint32_t flags = w_ld16(X, 52 - 48), ciaddr = w_ld32(X, 54 - 48);
    if ((flags & 0x8000) || ciaddr == 0) {
      rg_st16(c, 0, 0xFFFFu); rg_st32(c, 2, 0xFFFFFFFFu);
      bcast = true;
    } else {
      rg_st16(c, 0, w_ld16(X, 70 - 48)); rg_st32(c, 2, w_ld32(X, 72 - 48));
    }
    dst_ip = 0xFFFFFFFFu; dport = 68;
  }
  rg_st16(c, 6, smac_hi); rg_st32(c, 8, smac_lo);
  rg_st32(c, 26, R.server_ip); rg_st32(c, 30, dst_ip);
  rg_st16(c, 34, 67); rg_st16(c, 36, dport);
  rg_st8(c, 22, 64);                  /* TTL */
  rg_st16(c, 40, 0);                  /* UDP csum 0 (ref :741,755) */
  rg_st8(c, 42, 2);                   /* BOOTREPLY */
  rg_st8(c, 45, 0);                   /* hops */
  rg_st16(c, 16, 20 + 8 + 240 + w);   /* IP total length */
  rg_st16(c, 38, 8 + 240 + w);        /* UDP length */
  rg_st16(c, 24, 0);
  /* 10x u16 sum over bytes 14..33, from the window */
  uint32_t s = 0;
  #pragma unroll
  for (int i = 0; i < 10; ++i) s += rg_ld16(c, 14 + 2 * i);
  s = (s & 0xFFFF) + (s >> 16); s = (s & 0xFFFF) + (s >> 16);
  rg_st16(c, 24, ~s & 0xFFFFu);

  w_st32(X, 58 - 48, R.yiaddr);
  w_st32(X, 62 - 48, R.server_ip);
  w_st16(X, 86 - 48, 0); X[10] = 0; X[11] = 0;   /* sname 86..95 */

  uint4* q = (uint4*)p;
  q[0] = w_chunk(c.W, 0); q[1] = w_chunk(c.W, 1); q[2] = w_chunk(c.W, 2);
  q[3] = w_chunk(X, 0); q[4] = w_chunk(X, 1); q[5] = w_chunk(X, 2);
  #pragma unroll
  for (int i = 6; i < 17; ++i) q[i] = make_uint4(0, 0, 0, 0);   /* ..271 */
  if (ndns == 0) dhcp_wide_options<0>(p, R, pool);
  else if (ndns == 1) dhcp_wide_options<1>(p, R, pool);
  else dhcp_wide_options<2>(p, R, pool);
  return BNG_DHCP_OPT_OFF + w;
}

/* Per-packet DHCP fast path on an already parsed frame (`parsed` is
 * parse_pkt's result).  Returns verdict; *out_len set on TX. */
BNG_DEV int dhcp_process_ctx(pktctx& c, bool parsed, int stride,
                             const dhcp_tables& T, dhcp_flags& F,
                             uint16_t* out_len) {
  uint8_t* p = c.p;
  const int len = c.len;
  *out_len = (uint16_t)len;
  if (!parsed) {
    if (c.tagged) F.vlan = true;
    return BNG_PASS;
  }
  if (c.tagged) F.vlan = true;
  if (c.ip_off < 0 || c.proto != 17 || !c.l4_ok) return BNG_PASS;
  if (c.dport != 67) return BNG_PASS;
  int dhcp_off = c.l4_off + 8;
  if (len < dhcp_off + 240) return BNG_PASS;
  /* wide: constant offsets, row long enough for the longest reply */
  const bool wide = c.regs && stride >= BNG_DHCP_WIDE_MIN_STRIDE;
  uint32_t X[12];                    /* bytes 48..95 when wide */
  #pragma unroll
  for (int i = 0; i < 12; ++i) X[i] = 0;
  if (wide) {
    if (RG_B(c, 42) != 1) return BNG_PASS;             /* BOOTREQUEST */
    const uint4* q = (const uint4*)p;
    uint4 m = q[17];                 /* 272..287: cookie at 278..281 */
    uint32_t cookie = (__builtin_bswap32(m.y) << 16) |
                      (__builtin_bswap32(m.z) >> 16);
    if (cookie != 0x63825363u) return BNG_PASS;
    #pragma unroll
    for (int i = 0; i < 3; ++i) {
      uint4 v = q[3 + i];
      X[i * 4 + 0] = __builtin_bswap32(v.x);
      X[i * 4 + 1] = __builtin_bswap32(v.y);
      X[i * 4 + 2] = __builtin_bswap32(v.z);
      X[i * 4 + 3] = __builtin_bswap32(v.w);
    }
  } else {
    if (p[dhcp_off] != 1) return BNG_PASS;             /* BOOTREQUEST */
    if (ld_u32be(p + dhcp_off + 236) != 0x63825363u) return BNG_PASS;
  }

  F.total = true;

  uint8_t msg_type; const uint8_t* cid; int cid_len;
  scan_dhcp_options(p, dhcp_off + 240, len, &msg_type, &cid, &cid_len);
  if (msg_type != 1 && msg_type != 3) { F.miss = true; return BNG_PASS; }

  /* 3-way lookup: VLAN -> circuit-id -> MAC (ref :647-687) */
  const bng_sub_entry* sub = nullptr;
  if (c.tagged) {
    uint64_t vk = BNG_KEY_VLAN | ((uint64_t)c.s_tag << 16) | c.c_tag;
    sub = sub_lookup(T.subs, T.sub_mask, vk);
  }
  if (!sub && cid) {
    /* FNV-1a over the circuit-id zero-padded to 32 bytes, hashed as it
     * is read (a padded copy would live in scratch memory) */
    uint64_t h = 0xCBF29CE484222325ULL;
    for (int i = 0; i < 32; ++i) {
      h ^= (i < cid_len) ? cid[i] : 0;
      h *= 0x100000001B3ULL;
    }
    uint64_t ck = BNG_KEY_CIRCUIT | (h >> 2);
    sub = sub_lookup(T.subs, T.sub_mask, ck);
    if (sub) F.o82 = true;
  }
  if (!sub) {
    uint64_t mac = 0;
    if (wide) {
      mac = ((uint64_t)w_ld16(X, 70 - 48) << 32) | w_ld32(X, 72 - 48);
    } else {
      #pragma unroll
      for (int i = 0; i < 6; ++i) mac = (mac << 8) | p[dhcp_off + 28 + i];
    }
    sub = sub_lookup(T.subs, T.sub_mask, mac);
  }
  if (!sub) { F.miss = true; return BNG_PASS; }
  if (T.now_sec > sub->lease_expiry) { F.expired = true; return BNG_PASS; }
  if (sub->pool_id >= T.n_pools) { F.error = true; return BNG_PASS; }
  const bng_ip_pool pool = T.pools[sub->pool_id];
  if (!pool.valid) { F.error = true; return BNG_PASS; }
  F.hit = true;

  const bng_server_config cfg = *T.cfg;
  uint8_t reply_type = (msg_type == 1) ? 2 : 5;     /* OFFER : ACK */
  /* table IPs are stored as host ints equal to their wire (big-endian)
   * interpretation — the same values ip2u32()/ld_u32be() produce */
  uint32_t server_ip = cfg.server_ip ? cfg.server_ip : pool.gateway;
  if (wide) {
    dhcp_reply R{sub->allocated_ip, server_ip, reply_type};
    bool wbcast;
    int total = dhcp_reply_wide(c, X, R, pool, cfg, wbcast);
    F.bcast = wbcast; F.ucast = !wbcast;
    *out_len = (uint16_t)min(total, stride);
    return BNG_TX;
  }
  uint32_t giaddr = ld_u32be(p + dhcp_off + 24);
  bool bcast = false;

  int ip_off = c.ip_off, udp_off = c.l4_off;
  if (giaddr != 0) {   /* relayed: unicast to relay agent (ref :726-743) */
    #pragma unroll
    for (int i = 0; i < 6; ++i) p[i] = p[6 + i];
    #pragma unroll
    for (int i = 0; i < 6; ++i) p[6 + i] = cfg.server_mac[i];
    st_u32be(p + ip_off + 12, server_ip);
    st_u32be(p + ip_off + 16, giaddr);
    st_u16be(p + udp_off, 67); st_u16be(p + udp_off + 2, 67);
  } else {
    uint16_t flags = ld_u16be(p + dhcp_off + 10);
    uint32_t ciaddr = ld_u32be(p + dhcp_off + 12);
    bcast = (flags & 0x8000) || ciaddr == 0;
    if (bcast) {
      #pragma unroll
      for (int i = 0; i < 6; ++i) p[i] = 0xFF;
    } else {
      #pragma unroll
      for (int i = 0; i < 6; ++i) p[i] = p[dhcp_off + 28 + i];
    }
    #pragma unroll
    for (int i = 0; i < 6; ++i) p[6 + i] = cfg.server_mac[i];
    st_u32be(p + ip_off + 12, server_ip);
    st_u32be(p + ip_off + 16, 0xFFFFFFFFu);
    st_u16be(p + udp_off, 67); st_u16be(p + udp_off + 2, 68);
  }
  p[ip_off + 8] = 64;                 /* TTL */
  st_u16be(p + udp_off + 6, 0);       /* UDP csum 0 (ref :741,755) */

  p[dhcp_off] = 2;                    /* BOOTREPLY */
  p[dhcp_off + 3] = 0;                /* hops */
  st_u32be(p + dhcp_off + 16, sub->allocated_ip);
  st_u32be(p + dhcp_off + 20, server_ip);
  bng_zero(p + dhcp_off + 44, 192);   /* sname + file (ref :765-766) */

  /* options 53/54/51/1/3/6/58/59/255 (ref build_dhcp_options :519-602) */
  uint8_t* o = p + dhcp_off + 240;
  int w = 0;
  o[w++] = 53; o[w++] = 1; o[w++] = reply_type;
  o[w++] = 54; o[w++] = 4; st_u32be(o + w, server_ip); w += 4;
  o[w++] = 51; o[w++] = 4; st_u32be(o + w, pool.lease_time); w += 4;
  o[w++] = 1;  o[w++] = 4; st_u32be(o + w, pool_netmask(pool)); w += 4;
  o[w++] = 3;  o[w++] = 4; st_u32be(o + w, pool.gateway); w += 4;
  if (pool.dns_primary) {
    uint8_t dl = pool.dns_secondary ? 8 : 4;
    o[w++] = 6; o[w++] = dl;
    st_u32be(o + w, pool.dns_primary); w += 4;
    if (pool.dns_secondary) { st_u32be(o + w, pool.dns_secondary); w += 4; }
  }
  o[w++] = 58; o[w++] = 4; st_u32be(o + w, pool.lease_time / 2); w += 4;
  o[w++] = 59; o[w++] = 4; st_u32be(o + w, (pool.lease_time * 7) / 8); w += 4;
  o[w++] = 255;

  int dhcp_len = 240 + w;
  int udp_len = 8 + dhcp_len;
  int ip_len = 20 + udp_len;
  int total = 14 + c.vlan_offset + ip_len;
  st_u16be(p + ip_off + 2, (uint16_t)ip_len);
  st_u16be(p + udp_off + 4, (uint16_t)udp_len);
  st_u16be(p + ip_off + 10, 0);
  /* 10x u16 sum checksum (ref ip_checksum :488-503) */
  uint32_t s = 0;
  #pragma unroll
  for (int i = 0; i < 10; ++i) s += ld_u16be(p + ip_off + 2 * i);
  s = (s & 0xFFFF) + (s >> 16); s = (s & 0xFFFF) + (s >> 16);
  st_u16be(p + ip_off + 10, (uint16_t)~s);

  F.bcast = bcast; F.ucast = !bcast;
  *out_len = (uint16_t)min(total, stride);
  return BNG_TX;
}

/* parse + process, for the kernels that see nothing but DHCP */
BNG_DEV int dhcp_process(uint8_t* p, int len, int stride,
                         const dhcp_tables& T, dhcp_flags& F,
                         uint16_t* out_len) {
  pktctx c;
  bool parsed = parse_pkt(c, p, len, /*want_vlan=*/true);
  return dhcp_process_ctx(c, parsed, stride, T, F, out_len);
}

/* Layout of the per-block shared counter array the batched packet kernels
 * aggregate into (bng_device.h sb_*): the four global stat arrays back to
 * back, each group in its ABI enum order. */
enum {
  SB_DHCP = 0,
  SB_NAT = SB_DHCP + BNG_DHCP_NSTATS,
  SB_AS = SB_NAT + BNG_NAT_NSTATS,
  SB_QOS = SB_AS + BNG_AS_NSTATS,
  SB_N = SB_QOS + BNG_QOS_NSTATS
};

/* end of one grid-stride iteration: count each flag over the wave and
 * add it to the block's shared counters */
BNG_DEV void dhcp_count_stats(const dhcp_flags& F, unsigned long long* sb) {
  sb_fold(sb, SB_DHCP + BNG_ST_VLAN_PACKETS, wave_count(F.vlan));
  sb_fold(sb, SB_DHCP + BNG_ST_TOTAL_REQUESTS, wave_count(F.total));
  sb_fold(sb, SB_DHCP + BNG_ST_FASTPATH_HITS, wave_count(F.hit));
  sb_fold(sb, SB_DHCP + BNG_ST_FASTPATH_MISSES, wave_count(F.miss));
  sb_fold(sb, SB_DHCP + BNG_ST_CACHE_EXPIRED, wave_count(F.expired));
  sb_fold(sb, SB_DHCP + BNG_ST_ERRORS, wave_count(F.error));
  sb_fold(sb, SB_DHCP + BNG_ST_OPTION82_PRESENT, wave_count(F.o82));
  sb_fold(sb, SB_DHCP + BNG_ST_BROADCAST_REPLIES, wave_count(F.bcast));
  sb_fold(sb, SB_DHCP + BNG_ST_UNICAST_REPLIES, wave_count(F.ucast));
}

/* per-wave commit: the persistent service publishes per served batch */
BNG_DEV void dhcp_commit_stats(const dhcp_flags& F, unsigned long long* st) {
  stat_inc(&st[BNG_ST_VLAN_PACKETS], F.vlan);
  stat_inc(&st[BNG_ST_TOTAL_REQUESTS], F.total);
  stat_inc(&st[BNG_ST_FASTPATH_HITS], F.hit);
  stat_inc(&st[BNG_ST_FASTPATH_MISSES], F.miss);
  stat_inc(&st[BNG_ST_CACHE_EXPIRED], F.expired);
  stat_inc(&st[BNG_ST_ERRORS], F.error);
  stat_inc(&st[BNG_ST_OPTION82_PRESENT], F.o82);
  stat_inc(&st[BNG_ST_BROADCAST_REPLIES], F.bcast);
  stat_inc(&st[BNG_ST_UNICAST_REPLIES], F.ucast);
}

__global__ void dhcp_fastpath_kernel(
    uint8_t* __restrict__ data, const uint16_t* __restrict__ in_len,
    uint16_t* __restrict__ out_len, uint8_t* __restrict__ verdict,
    int n, int stride,
    const bng_sub_entry* __restrict__ subs, uint32_t sub_mask,
    const bng_ip_pool* __restrict__ pools, uint32_t n_pools,
    const bng_server_config* __restrict__ cfg,
    unsigned long long* __restrict__ stats, uint64_t now_sec,
    const uint64_t* __restrict__ now_ptr) {
  if (now_ptr) now_sec = now_ptr[1];
  dhcp_tables T{subs, sub_mask, pools, n_pools, cfg, stats, now_sec};
  __shared__ unsigned long long sb[SB_N];
  sb_zero(sb, SB_N);
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int base = 0; base < n; base += nthreads) {
    int pid = base + tid;
    dhcp_flags F; F.clear();
    if (pid < n) {
      uint16_t ol = in_len[pid];
      int v = dhcp_process(data + (size_t)pid * stride, in_len[pid], stride,
                           T, F, &ol);
      verdict[pid] = (uint8_t)v;
      out_len[pid] = ol;
    }
    dhcp_count_stats(F, sb);
  }
  __syncthreads();
  sb_commit(sb, SB_DHCP, BNG_DHCP_NSTATS, stats);
}

/* ------------------------------------------- persistent DHCP service.
 * One workgroup (256 threads, 1 CU of 256) stays resident and polls a
 * pinned-host doorbell.  Because its waves already occupy their CU, a
 * saturating 1M-packet data flood cannot starve it the way it starves
 * a freshly launched kernel (measured r1: flood p99 453 us vs <70 us
 * quiesced; a priority stream did not help because the launch itself
 * must wait for CU space).  Request path: host writes packets into the
 * pinned ring and bumps head; the kernel stages the batch to an HBM
 * scratch with wide coalesced PCIe reads, runs dhcp_process, copies
 * replies back, and release-stores tail.  Self-exits after
 * idle_exit_k*1024 empty polls so a crashed host can never wedge the
 * box. */
/* Multi-block service: each block owns a fixed slice of the batch and
 * polls the doorbell independently (no grid sync).  Spreading the
 * slices over N CUs multiplies the outstanding PCIe reads during
 * staging (the single-block form measured latency-bound at ~68 us for
 * a 256-pkt batch) and divides the per-CU work a saturating data flood
 * contends with.  Completion: the last block to finish a batch
 * (device-scope acq_rel counter) publishes tail; the last block to
 * exit publishes the exit ack. */
__global__ void __launch_bounds__(256, 1) dhcp_service_kernel(
    bng_svc_ctrl* __restrict__ ctrl,
    uint8_t* __restrict__ req,            /* pinned [n_slots, stride]  */
    const uint16_t* __restrict__ in_len,  /* pinned [n_slots]          */
    uint16_t* __restrict__ out_len,       /* pinned [n_slots]          */
    uint8_t* __restrict__ verdict,        /* pinned [n_slots]          */
    uint8_t* __restrict__ scratch,        /* device [n_slots, stride]  */
    int n_slots,
    uint32_t* __restrict__ ctrs,          /* device {done, served_lo,
                                             served_hi, exits}         */
    const bng_sub_entry* __restrict__ subs, uint32_t sub_mask,
    const bng_ip_pool* __restrict__ pools, uint32_t n_pools,
    const bng_server_config* __restrict__ cfg,
    unsigned long long* __restrict__ stats) {
  __shared__ uint32_t s_head, s_run, s_n;
  __shared__ uint64_t s_now;
  const int tid = threadIdx.x;
  const int nb = (int)gridDim.x, blk = (int)blockIdx.x;
  uint32_t done = __hip_atomic_load(&ctrl->tail, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_SYSTEM);
  const int stride = (int)ctrl->stride;
  uint64_t idle = 0;
  const uint64_t idle_max = (uint64_t)ctrl->idle_exit_k * 1024u;
  uint64_t batches = 0;
  unsigned long long* served64 = (unsigned long long*)(ctrs + 4);
  for (;;) {
    if (tid == 0) {
      s_head = __hip_atomic_load(&ctrl->head, __ATOMIC_ACQUIRE,
                                 __HIP_MEMORY_SCOPE_SYSTEM);
      s_run = __hip_atomic_load(&ctrl->run, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_SYSTEM);
      s_n = ctrl->n_pkts;
      s_now = ctrl->now_sec;
    }
    __syncthreads();
    bool work = (s_head != done);
    if (!s_run || (!work && idle >= idle_max)) break;
    if (!work) {
      ++idle;
      __builtin_amdgcn_s_sleep(8);
      __syncthreads();           /* re-converge before the next poll */
      continue;
    }
    idle = 0;
    int n = (int)s_n;
    if (n > n_slots) n = n_slots;
    const int lo = (int)((long)n * blk / nb);
    const int hi = (int)((long)n * (blk + 1) / nb);
    /* stage this block's slice to HBM: wide coalesced PCIe reads */
    const size_t w0 = (size_t)lo * stride / 16;
    const int words = (hi - lo) * stride / 16;
    const uint4* src = (const uint4*)req + w0;
    uint4* dst = (uint4*)scratch + w0;
    for (int i = tid; i < words; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
    dhcp_tables T{subs, sub_mask, pools, n_pools, cfg, stats, s_now};
    for (int pid = lo + tid; pid < hi; pid += blockDim.x) {
      dhcp_flags F; F.clear();
      uint16_t ol = in_len[pid];
      int v = dhcp_process(scratch + (size_t)pid * stride, in_len[pid],
                           stride, T, F, &ol);
      verdict[pid] = (uint8_t)v;
      out_len[pid] = ol;
      dhcp_commit_stats(F, stats);
    }
    __syncthreads();
    /* replies back to the pinned ring (posted PCIe writes) */
    for (int i = tid; i < words; i += blockDim.x)
      ((uint4*)req)[w0 + i] = dst[i];
    __syncthreads();
    ++done; ++batches;
    if (tid == 0) {
      atomicAdd(served64, (unsigned long long)(hi - lo));
      /* acq_rel: the winner observes every block's served add */
      uint32_t prev = __hip_atomic_fetch_add(&ctrs[0], 1u,
                                             __ATOMIC_ACQ_REL,
                                             __HIP_MEMORY_SCOPE_AGENT);
      if ((int)(prev % (uint32_t)nb) == nb - 1) {   /* last finisher */
        ctrl->served = *served64;
        ctrl->batches = batches;
        __hip_atomic_store(&ctrl->tail, done, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    uint32_t prev = __hip_atomic_fetch_add(&ctrs[1], 1u, __ATOMIC_ACQ_REL,
                                           __HIP_MEMORY_SCOPE_AGENT);
    if ((int)prev == nb - 1) {
      ctrl->served = *served64;
      /* exit ack: the host's stop() waits on this instead of a stream
       * sync, so a dead doorbell can never block the control plane */
      __hip_atomic_store(&ctrl->exited, 1u, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

/* ========================================================== NAT44  K2 */

struct nat_tables {
  bng_nat_session* sessions; uint32_t sess_mask;
  bng_nat_reverse* reverse;  uint32_t rev_mask;
  bng_eim_entry* eim;        uint32_t eim_mask;
  bng_subctx* ctx;           uint32_t ctx_mask;
  const bng_nat_config* cfg;
  const uint32_t* hairpin_ips; uint32_t n_hairpin;
  unsigned long long* stats;
  bng_nat_log_entry* log_ring; bng_ring_header* log_hdr;
  uint64_t now_ns;
};

struct nat_flags {
  bool snat, dnat, hairpin, dropped, passed, sess_created, sess_expired,
       port_exh, eim_hit, eim_miss, alg, icmp_xlate, icmp_nomap;
  BNG_DEV void clear() {
    snat = dnat = hairpin = dropped = passed = sess_created = sess_expired =
        port_exh = eim_hit = eim_miss = alg = icmp_xlate = icmp_nomap = false;
  }
};

/* membership over sorted disjoint intervals: binary search, O(log n)
 * (the LPM-trie equivalent for a membership query) */
BNG_DEV bool ip_in_intervals(const uint32_t* lo, const uint32_t* hi,
                             uint32_t n, uint32_t ip) {
  uint32_t l = 0, r = n;
  while (l < r) {
    uint32_t m = (l + r) >> 1;
    if (ip < lo[m]) r = m;
    else if (ip > hi[m]) l = m + 1;
    else return true;
  }
  return false;
}

BNG_DEV bool nat_is_private(const bng_nat_config* cfg, uint32_t ip) {
  return ip_in_intervals(cfg->priv_lo, cfg->priv_hi,
                         cfg->n_private_ranges, ip);
}

BNG_DEV bool nat_is_hairpin(const nat_tables& T, uint32_t ip) {
  for (uint32_t i = 0; i < T.n_hairpin; ++i)
    if (T.hairpin_ips[i] == ip) return true;
  return false;
}

BNG_DEV bool nat_is_alg(const bng_nat_config* cfg, uint16_t port,
                        uint8_t proto) {
  uint32_t key = ((uint32_t)port << 16) | proto;
  for (uint32_t i = 0; i < cfg->n_alg_ports; ++i)
    if (cfg->alg_key[i] == key) return true;
  return false;
}

BNG_DEV void nat_log_push(const nat_tables& T, uint32_t ev, uint32_t sub_id,
                          uint32_t priv_ip, uint32_t pub_ip,
                          uint16_t priv_port, uint16_t pub_port,
                          uint32_t dest_ip, uint16_t dest_port,
                          uint8_t proto, uint8_t flags) {
  if (!T.log_ring) return;
  uint32_t idx = ring_claim(T.log_hdr);
  bng_nat_log_entry* e = &T.log_ring[idx & ((1u << BNG_LOG_RING_LOG2) - 1)];
  e->timestamp = T.now_ns; e->event_type = ev; e->subscriber_id = sub_id;
  e->private_ip = priv_ip; e->public_ip = pub_ip;
  e->private_port = priv_port; e->public_port = pub_port;
  e->dest_ip = dest_ip; e->dest_port = dest_port;
  e->protocol = proto; e->flags = flags;
}

/* Port rotor (ref allocate_port_from_block nat44.c:408-466): take the
 * rotor's position, step it with the wrap, optional RTP parity,
 * EIM-collision heuristic.
 *
 * Position and wrap are ONE compare-and-swap on next_port.  The reference
 * bumps the counter and repairs the wrap afterwards, a race two CPUs have
 * to collide on; here the lanes of a wave get consecutive counter values
 * in lock-step, so every wave that crossed port_end handed port_start to
 * all of its lanes past the end (and, in a block ending at 65535, the
 * counter truncated to 16 bits came out as port 0 = "exhausted", then as
 * ports 1, 2, ... outside the block).  With the CAS k <= block-size
 * concurrent callers get k consecutive positions modulo the block size,
 * next_port never leaves [port_start, port_end], and any interleaving
 * gives what the sequential model gives.  The loop is lock-free: a failed
 * CAS means another caller's landed, so the retries of one caller are
 * bounded by the callers racing it, and the failed CAS returns the value
 * to retry with.  Only the session-create path comes here. */
BNG_DEV uint16_t nat_alloc_port(const nat_tables& T, bng_subctx* blk,
                                bool parity, uint16_t orig_port,
                                uint32_t internal_ip, uint8_t proto) {
  uint8_t orig_parity = orig_port & 1;
  const uint32_t first = blk->port_start, last = blk->port_end;
  uint32_t cur = rlx_load32(&blk->next_port);
  for (int i = 0; i < 64; ++i) {
    uint32_t pos, nxt;
    for (;;) {
      /* a position outside the block (a table image from elsewhere)
       * restarts the rotor instead of being handed out */
      pos = (cur >= first && cur <= last) ? cur : first;
      nxt = pos == last ? first : pos + 1;
      uint32_t seen = atomicCAS(&blk->next_port, cur, nxt);
      if (seen == cur) break;
      cur = seen;
    }
    cur = nxt;
    uint16_t port = (uint16_t)pos;
    if (parity && (port & 1) != orig_parity) continue;
    uint64_t esig = bng_eim_sig(internal_ip, port, proto);
    bng_eim_entry* ex = sig_lookup(T.eim, T.eim_mask, esig);
    if (ex) {
      /* verify it really is this (ip,port,proto) */
      if (bng_wait_ready(&ex->ready, 4096) && ex->internal_ip == internal_ip
          && ex->internal_port == port && ex->protocol == proto)
        continue;
    }
    return port;
  }
  return 0;
}

/* incremental checksum helpers (ref update_csum nat44.c:378-398) */
BNG_DEV uint16_t csum_upd32(uint16_t csum, uint32_t oldv, uint32_t newv) {
  uint32_t s = (~csum) & 0xFFFF;
  s += (~oldv & 0xFFFF) + ((~oldv >> 16) & 0xFFFF);
  s += (newv & 0xFFFF) + (newv >> 16);
  s = (s & 0xFFFF) + (s >> 16);
  s = (s & 0xFFFF) + (s >> 16);
  return (uint16_t)~s;
}
BNG_DEV uint16_t csum_upd16(uint16_t csum, uint16_t oldv, uint16_t newv) {
  uint32_t s = (~csum) & 0xFFFF;
  s += (~oldv & 0xFFFF) + newv;
  s = (s & 0xFFFF) + (s >> 16);
  s = (s & 0xFFFF) + (s >> 16);
  return (uint16_t)~s;
}

/* TCP/UDP/ICMP from a NATed subscriber that parsed without l4_ok (the rare
 * case, so the parser carries no flag for it and this looks again).  A
 * non-first fragment or a non-query ICMP message has nothing to key a
 * session on: the host slow path can reassemble and inspect, this one
 * cannot.  What is left ends inside its L4 header and is forwarded. */
BNG_DEV int nat_egress_no_l4(const pktctx& c, nat_flags& F) {
  const uint8_t* p = c.p;
  bool frag = (ld_u16be(p + c.ip_off + 6) & 0x1FFF) != 0;
  bool not_query = c.proto == 1 && c.len >= c.l4_off + 8 &&
                   !icmp_is_query(p[c.l4_off]);
  if (frag || not_query) { F.passed = true; return BNG_PASS; }
  return BNG_FWD;
}

/* SNAT (ref nat44_egress nat44.c:565-802) on an already-probed port
 * block: `blk` with its nat_valid flag as the probe saw it */
BNG_DEV int nat_egress_ctx(pktctx& c, const nat_tables& T, nat_flags& F,
                           bng_subctx* blk, bool nat_valid) {
  uint8_t* p = c.p;
  if (c.ip_off < 0) return BNG_FWD;
  const bng_nat_config* cfg = T.cfg;
  if (!nat_is_private(cfg, c.saddr)) return BNG_FWD;
  if (!blk || !nat_valid) { F.passed = true; return BNG_PASS; }

  uint16_t sport, dport;
  if (c.proto == 6) {
    if (!c.l4_ok) return nat_egress_no_l4(c, F);
    sport = c.sport; dport = c.dport;
    if (cfg->flags & (BNG_NAT_FLAG_ALG_FTP | BNG_NAT_FLAG_ALG_SIP)) {
      if (nat_is_alg(cfg, dport, 6)) {
        F.alg = true;
        nat_log_push(T, BNG_LOG_ALG_TRIGGER, blk->subscriber_id, c.saddr, 0,
                     sport, 0, c.daddr, dport, 6, 0);
        return BNG_PASS;
      }
    }
  } else if (c.proto == 17) {
    if (!c.l4_ok) return nat_egress_no_l4(c, F);
    sport = c.sport; dport = c.dport;
    if (cfg->flags & BNG_NAT_FLAG_ALG_SIP) {
      if (nat_is_alg(cfg, dport, 17)) {
        F.alg = true;
        nat_log_push(T, BNG_LOG_ALG_TRIGGER, blk->subscriber_id, c.saddr, 0,
                     sport, 0, c.daddr, dport, 17, 0);
        return BNG_PASS;
      }
    }
  } else if (c.proto == 1) {
    if (!c.l4_ok) return nat_egress_no_l4(c, F);
    sport = c.icmp_id; dport = 0;
  } else {
    return BNG_FWD;
  }

  uint8_t is_hairpin = 0;
  if ((cfg->flags & BNG_NAT_FLAG_HAIRPIN) && nat_is_hairpin(T, c.daddr)) {
    is_hairpin = 1; F.hairpin = true;
  }

  uint64_t sig = bng_tuple_sig(c.saddr, c.daddr, sport, dport, c.proto);
  const auto sr = sig_find_or_claim(T.sessions, T.sess_mask, sig);
  bng_nat_session* sess = sr.e;
  if (!sess) { F.passed = true; return BNG_PASS; }  /* table section full */

  uint32_t nat_ip; uint16_t nat_port;
  if (sr.found) {
    /* HIT fast path: the producer plain-stored fields then issued an
     * agent release (L2 write-back) before the sc1 `ready` store, so
     * relaxed agent (sc1, L2-served) loads are always fresh — no
     * acquire fence (which would flush this CU's whole L1) needed. */
    const uint64_t* e64 = (const uint64_t*)sess;
    uint64_t k0 = rlx_load64(e64 + 1);   /* src_ip | dst_ip<<32 */
    uint64_t k1 = rlx_load64(e64 + 2);   /* sport | dport<<16 | proto<<32 */
    uint64_t t0 = rlx_load64(e64 + 3);   /* nat_ip | nat_port<<32 | orig_port<<48 */
    uint64_t t1 = rlx_load64(e64 + 4);   /* orig_ip | state<<32 | hairpin<<40 | ready<<48 */
    if (!((t1 >> 48) & 0xFF)) {          /* creation still in flight */
      if (!bng_wait_ready(&sess->ready, 8192)) {
        F.passed = true; return BNG_PASS;
      }
      k0 = rlx_load64(e64 + 1); k1 = rlx_load64(e64 + 2);
      t0 = rlx_load64(e64 + 3); t1 = rlx_load64(e64 + 4);
    }
    uint64_t ek0 = ((uint64_t)c.daddr << 32) | c.saddr;
    uint64_t ek1 = (uint64_t)sport | ((uint64_t)dport << 16) |
                   ((uint64_t)c.proto << 32);
    if (k0 != ek0 || (k1 & 0xFFFFFFFFFFull) != ek1) {
      /* sig collision with a different tuple: slow path (rare) */
      F.passed = true; return BNG_PASS;
    }
    nat_ip = (uint32_t)t0;
    nat_port = (uint16_t)(t0 >> 32);
    /* one fabric store per batch per session, not per packet */
    if (rlx_load64(e64 + 5) != T.now_ns)
      rlx_store64((void*)(e64 + 5), T.now_ns);
    /* one packed accounting atomic: bytes<<24 | packets (folded into the
     * u64 counters by the sweep kernel) */
    atomicAdd((unsigned long long*)(e64 + 11),
              ((unsigned long long)c.len << 24) | 1ull);
  } else {
    /* we claimed the slot: allocate mapping (EIM or fresh port) */
    bool parity = (cfg->flags & BNG_NAT_FLAG_PARITY) != 0;
    bool have = false;
    if (cfg->flags & BNG_NAT_FLAG_EIM) {
      uint64_t esig = bng_eim_sig(c.saddr, sport, c.proto);
      const auto er = sig_find_or_claim(T.eim, T.eim_mask, esig);
      bng_eim_entry* eim = er.e;
      if (eim && er.found) {
        if (bng_wait_ready(&eim->ready, 8192) && eim->internal_ip == c.saddr
            && eim->internal_port == sport && eim->protocol == c.proto) {
          __hip_atomic_store(&eim->last_used, T.now_ns, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          atomicAdd(&eim->ref_count, 1u);
          F.eim_hit = true;
          nat_ip = eim->external_ip; nat_port = eim->external_port;
          have = true;
        }
      } else if (eim && er.claimed) {
        uint16_t ap = nat_alloc_port(T, blk, parity, sport, c.saddr, c.proto);
        if (ap == 0) {
          /* release the claimed EIM slot as tombstone, drop the packet */
          __hip_atomic_store(&eim->sig, BNG_KEY_TOMBSTONE, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(&sess->sig, BNG_KEY_TOMBSTONE, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          F.port_exh = true; F.dropped = true;
          nat_log_push(T, BNG_LOG_PORT_EXHAUSTION, blk->subscriber_id,
                       c.saddr, blk->public_ip, sport, 0, c.daddr, dport,
                       c.proto, 0);
          return BNG_DROP;
        }
        eim->internal_ip = c.saddr; eim->internal_port = sport;
        eim->protocol = c.proto;
        eim->external_ip = blk->public_ip;
        eim->external_port = ap;
        eim->created = T.now_ns; eim->last_used = T.now_ns;
        eim->ref_count = 1; eim->flags = 0;
        bng_publish_ready(&eim->ready);
        F.eim_miss = true;
        nat_ip = eim->external_ip;
        nat_port = ap;
        have = true;
      }
    }
    if (!have) {
      uint16_t ap = nat_alloc_port(T, blk, parity, sport, c.saddr, c.proto);
      if (ap == 0) {
        __hip_atomic_store(&sess->sig, BNG_KEY_TOMBSTONE, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        F.port_exh = true; F.dropped = true;
        nat_log_push(T, BNG_LOG_PORT_EXHAUSTION, blk->subscriber_id, c.saddr,
                     blk->public_ip, sport, 0, c.daddr, dport, c.proto, 0);
        return BNG_DROP;
      }
      nat_ip = blk->public_ip;
      nat_port = ap;
    }
    /* fill the session (ref :711-730) */
    sess->key = bng_nat_tuple{c.saddr, c.daddr, sport, dport, c.proto, {0,0,0}};
    sess->nat_ip = nat_ip; sess->nat_port = nat_port; sess->orig_port = sport;
    sess->orig_ip = c.saddr; sess->state = BNG_NAT_NEW;
    sess->is_hairpin = is_hairpin;
    sess->last_seen = T.now_ns; sess->created = T.now_ns;
    sess->packets_out = 1; sess->packets_in = 0;
    sess->bytes_out = c.len; sess->bytes_in = 0;
    bng_publish_ready(&sess->ready);

    /* reverse mapping for DNAT (ref :732-740) */
    uint64_t rsig = bng_tuple_sig(c.daddr, nat_ip, dport, nat_port, c.proto);
    const auto rr = sig_find_or_claim(T.reverse, T.rev_mask, rsig);
    bng_nat_reverse* rev = rr.e;
    if (rev && rr.claimed) {
      rev->key = bng_nat_tuple{c.daddr, nat_ip, dport, nat_port, c.proto,
                               {0, 0, 0}};
      rev->orig = sess->key;
      bng_publish_ready(&rev->ready);
    }
    atomicAdd(&blk->sessions_active, 1u);
    atomicAdd(&blk->sessions_total, 1u);
    F.sess_created = true;
    nat_log_push(T, BNG_LOG_SESSION_CREATE, blk->subscriber_id, c.saddr,
                 nat_ip, sport, nat_port, c.daddr, dport, c.proto,
                 is_hairpin);
  }

  /* SNAT rewrite + incremental checksums (ref :752-798).  When the
   * fast parse ran (c.regs: untagged ihl=5, fixed offsets 14/34) the
   * rewrite happens on the register window and flushes as two dwordx4
   * stores — the TA unit is the measured kernel bound and this path
   * replaces ~10 divergent byte R/W ops with 2 wide stores (the TCP
   * checksum at byte 50 stays in memory: outside the 48-B window). */
  uint32_t old_ip = c.saddr;
  uint16_t nat_port_host = nat_port;
  if (c.regs) {
    rg_st32(c, 26, nat_ip);
    rg_st16(c, 24, csum_upd32(rg_ld16(c, 24), old_ip, nat_ip));
    if (c.proto == 6) {
      uint16_t old_port = rg_ld16(c, 34);
      rg_st16(c, 34, nat_port_host);
      uint16_t ck = ld_u16be(p + 50);
      ck = csum_upd32(ck, old_ip, nat_ip);
      ck = csum_upd16(ck, old_port, nat_port_host);
      rg_flush16_47(c);
      st_u16be(p + 50, ck);
    } else if (c.proto == 17) {
      uint16_t old_port = rg_ld16(c, 34);
      rg_st16(c, 34, nat_port_host);
      uint16_t ck = rg_ld16(c, 40);
      if (ck != 0) {
        ck = csum_upd32(ck, old_ip, nat_ip);
        ck = csum_upd16(ck, old_port, nat_port_host);
        if (ck == 0) ck = 0xFFFF;
        rg_st16(c, 40, ck);
      }
      rg_flush16_47(c);
    } else {            /* ICMP: id at 38, checksum at 36 */
      uint16_t old_id = rg_ld16(c, 38);
      rg_st16(c, 38, nat_port_host);
      rg_st16(c, 36, csum_upd16(rg_ld16(c, 36), old_id, nat_port_host));
      rg_flush16_47(c);
    }
    F.snat = true;
    return BNG_FWD;
  }
  st_u32be(p + c.ip_off + 12, nat_ip);
  uint16_t ipck = ld_u16be(p + c.ip_off + 10);
  st_u16be(p + c.ip_off + 10, csum_upd32(ipck, old_ip, nat_ip));
  if (c.proto == 6) {
    uint16_t old_port = ld_u16be(p + c.l4_off);
    st_u16be(p + c.l4_off, nat_port_host);
    uint16_t ck = ld_u16be(p + c.l4_off + 16);
    ck = csum_upd32(ck, old_ip, nat_ip);
    ck = csum_upd16(ck, old_port, nat_port_host);
    st_u16be(p + c.l4_off + 16, ck);
  } else if (c.proto == 17) {
    uint16_t old_port = ld_u16be(p + c.l4_off);
    st_u16be(p + c.l4_off, nat_port_host);
    uint16_t ck = ld_u16be(p + c.l4_off + 6);
    if (ck != 0) {
      ck = csum_upd32(ck, old_ip, nat_ip);
      ck = csum_upd16(ck, old_port, nat_port_host);
      if (ck == 0) ck = 0xFFFF;
      st_u16be(p + c.l4_off + 6, ck);
    }
  } else if (c.proto == 1) {
    uint16_t old_id = ld_u16be(p + c.l4_off + 4);
    st_u16be(p + c.l4_off + 4, nat_port_host);
    uint16_t ck = ld_u16be(p + c.l4_off + 2);
    st_u16be(p + c.l4_off + 2, csum_upd16(ck, old_id, nat_port_host));
  }
  F.snat = true;
  return BNG_FWD;
}

/* the stand-alone form probes the port block itself */
BNG_DEV int nat_egress_process(pktctx& c, const nat_tables& T,
                               nat_flags& F) {
  if (c.ip_off < 0) return BNG_FWD;
  if (!nat_is_private(T.cfg, c.saddr)) return BNG_FWD;
  ctx_hit h = subctx_lookup(T.ctx, T.ctx_mask, c.saddr, /*want_qos=*/false);
  return nat_egress_ctx(c, T, F, h.e, h.nat_valid);
}

/* What nat_ingress_icmp_error did with the frame */
enum { ICMP_ERR_IGNORED = 0, ICMP_ERR_XLATE = 1, ICMP_ERR_NOMAP = 2 };

/* Inbound ICMP error to a public address (RFC 5508 REQ-3/4/5; no reference
 * analog: nat44.c:644-648 reads bytes 4..5 of an error as an echo id).  A
 * Destination Unreachable (3), Time Exceeded (11) or Parameter Problem (12)
 * quotes the datagram it is about, as the NAT sent it: the quoted source is
 * the public address and port.  The quote's flow is looked up the way DNAT
 * looks up a reply (reverse entry -> session), then the outer destination
 * and the quoted source address and port (or query id) become the
 * subscriber's, with every checksum that covers a changed word updated
 * incrementally — the quoted IP header's, the quoted L4's where its field
 * is inside the frame, and the outer ICMP's for each of those words.
 *
 * Reads the tables, writes none: an error neither refreshes last_seen nor
 * counts as session traffic, moves no TCP state and tombstones no stale
 * reverse entry (the next ordinary packet does that).  Every load and store
 * is a byte access below `len`.
 *
 * Cold (one call per error frame), so a real call, out of line: the DNAT
 * hit path keeps its registers.  The arguments are values on purpose — a
 * reference to the parsed context or to the flags would take their address
 * and put the context's register window into scratch memory in both
 * callers.  Returns ICMP_ERR_*; IGNORED is every frame this stage forwards
 * unread today and still does (a non-first fragment, fewer than 8 bytes of
 * ICMP, any other type). */
__device__ __noinline__ int nat_ingress_icmp_error(
    uint8_t* p, int len, int ip_off, int l4_off, uint32_t daddr,
    bng_nat_reverse* reverse, uint32_t rev_mask,
    bng_nat_session* sessions, uint32_t sess_mask) {
  if (ld_u16be(p + ip_off + 6) & 0x1FFF) return ICMP_ERR_IGNORED;
  if (len < l4_off + 8) return ICMP_ERR_IGNORED;
  uint32_t type = p[l4_off];
  if (type != 3 && type != 11 && type != 12) return ICMP_ERR_IGNORED;

  /* the quoted datagram: header at e, its first 8 L4 bytes at q */
  int e = l4_off + 8;
  if (len < e + 20) return ICMP_ERR_NOMAP;
  uint32_t vihl = p[e];
  if ((vihl >> 4) != 4 || (vihl & 0xF) < 5) return ICMP_ERR_NOMAP;
  int q = e + (int)(vihl & 0xF) * 4;
  if (len < q + 8) return ICMP_ERR_NOMAP;
  if (ld_u16be(p + e + 6) & 0x1FFF) return ICMP_ERR_NOMAP;
  uint32_t pub_ip = ld_u32be(p + e + 12), remote_ip = ld_u32be(p + e + 16);
  if (pub_ip != daddr) return ICMP_ERR_NOMAP;
  uint32_t proto = p[e + 9];
  int id_at;                       /* the public port or id inside the quote */
  uint16_t sport;                  /* reverse key: the remote end's port */
  if (proto == 6 || proto == 17) {
    id_at = q; sport = ld_u16be(p + q + 2);
  } else if (proto == 1 && icmp_is_query(p[q])) {
    id_at = q + 4; sport = 0;
  } else return ICMP_ERR_NOMAP;
  uint16_t pub_port = ld_u16be(p + id_at);

  /* reverse entry -> session, with DNAT's checks and none of its writes */
  uint64_t rsig = bng_tuple_sig(remote_ip, pub_ip, sport, pub_port,
                                (uint8_t)proto);
  bng_nat_reverse* rev = sig_lookup(reverse, rev_mask, rsig);
  if (!rev || !bng_wait_ready(&rev->ready, 8192)) return ICMP_ERR_NOMAP;
  const uint64_t* r64 = (const uint64_t*)rev;
  uint64_t k0 = rlx_load64(r64 + 1), k1 = rlx_load64(r64 + 2);
  uint64_t ek0 = ((uint64_t)pub_ip << 32) | remote_ip;
  uint64_t ek1 = (uint64_t)sport | ((uint64_t)pub_port << 16) |
                 ((uint64_t)proto << 32);
  if (k0 != ek0 || (k1 & 0xFFFFFFFFFFull) != ek1) return ICMP_ERR_NOMAP;
  bng_nat_tuple orig;
  uint64_t o0 = rlx_load64(r64 + 3), o1 = rlx_load64(r64 + 4);
  orig.src_ip = (uint32_t)o0; orig.dst_ip = (uint32_t)(o0 >> 32);
  orig.src_port = (uint16_t)o1; orig.dst_port = (uint16_t)(o1 >> 16);
  orig.protocol = (uint8_t)(o1 >> 32);
  uint64_t osig = bng_tuple_sig(orig.src_ip, orig.dst_ip, orig.src_port,
                                orig.dst_port, orig.protocol);
  const bng_nat_session* sess = sig_lookup(sessions, sess_mask, osig);
  if (!sess || !bng_wait_ready(&sess->ready, 8192) ||
      !tuple_eq(sess->key, orig))
    return ICMP_ERR_NOMAP;
  uint32_t new_ip = sess->orig_ip;
  uint16_t new_port = sess->orig_port;

  /* 1. outer destination, outer header checksum */
  st_u32be(p + ip_off + 16, new_ip);
  st_u16be(p + ip_off + 10,
           csum_upd32(ld_u16be(p + ip_off + 10), pub_ip, new_ip));
  /* the outer ICMP checksum follows every quoted word that changes */
  uint16_t ock = ld_u16be(p + l4_off + 2);
  /* 2. quoted source, quoted header checksum */
  st_u32be(p + e + 12, new_ip);
  ock = csum_upd32(ock, pub_ip, new_ip);
  {
    uint16_t ck = ld_u16be(p + e + 10);
    uint16_t nk = csum_upd32(ck, pub_ip, new_ip);
    st_u16be(p + e + 10, nk);
    ock = csum_upd16(ock, ck, nk);
  }
  /* 3. quoted source port or id */
  st_u16be(p + id_at, new_port);
  ock = csum_upd16(ock, pub_port, new_port);
  /* 4. quoted L4 checksum, where the quote reaches it */
  int ck_at = proto == 6 ? q + 16 : proto == 17 ? q + 6 : q + 2;
  if (len >= ck_at + 2) {
    uint16_t ck = ld_u16be(p + ck_at), nk = ck;
    if (proto == 1) {
      nk = csum_upd16(ck, pub_port, new_port);
    } else if (proto == 6 || ck != 0) {      /* UDP 0: sender computed none */
      nk = csum_upd32(ck, pub_ip, new_ip);
      nk = csum_upd16(nk, pub_port, new_port);
      if (proto == 17 && nk == 0) nk = 0xFFFF;
    }
    if (nk != ck) {
      st_u16be(p + ck_at, nk);
      ock = csum_upd16(ock, ck, nk);
    }
  }
  /* 5. outer ICMP checksum */
  st_u16be(p + l4_off + 2, ock);
  return ICMP_ERR_XLATE;
}

/* DNAT (ref nat44_ingress nat44.c:805-948) */
BNG_DEV int nat_ingress_process(pktctx& c, const nat_tables& T, nat_flags& F) {
  uint8_t* p = c.p;
  if (c.ip_off < 0) return BNG_FWD;
  uint16_t sport, dport;
  if (c.proto == 6 || c.proto == 17) {
    if (!c.l4_ok) return BNG_FWD;
    sport = c.sport; dport = c.dport;
  } else if (c.proto == 1) {
    if (!c.l4_ok) {
      if (T.cfg->flags & BNG_NAT_FLAG_ICMP_ERR) {
        int r = nat_ingress_icmp_error(p, c.len, c.ip_off, c.l4_off, c.daddr,
                                       T.reverse, T.rev_mask, T.sessions,
                                       T.sess_mask);
        F.icmp_xlate = r == ICMP_ERR_XLATE;
        F.icmp_nomap = r == ICMP_ERR_NOMAP;
      }
      return BNG_FWD;
    }
    sport = 0; dport = c.icmp_id;
  } else return BNG_FWD;

  uint64_t rsig = bng_tuple_sig(c.saddr, c.daddr, sport, dport, c.proto);
  bng_nat_reverse* rev = sig_lookup(T.reverse, T.rev_mask, rsig);
  if (!rev) { F.passed = true; return BNG_FWD; }
  {
    const uint64_t* r64 = (const uint64_t*)rev;
    uint64_t rdy = rlx_load64(r64 + 5);      /* ready at byte 40 */
    if (!(rdy & 0xFF) && !bng_wait_ready(&rev->ready, 8192)) {
      F.passed = true; return BNG_FWD;
    }
    uint64_t k0 = rlx_load64(r64 + 1), k1 = rlx_load64(r64 + 2);
    uint64_t ek0 = ((uint64_t)c.daddr << 32) | c.saddr;
    uint64_t ek1 = (uint64_t)sport | ((uint64_t)dport << 16) |
                   ((uint64_t)c.proto << 32);
    if (k0 != ek0 || (k1 & 0xFFFFFFFFFFull) != ek1) {
      F.passed = true; return BNG_FWD;
    }
  }
  bng_nat_tuple orig;
  {
    const uint64_t* r64 = (const uint64_t*)rev;
    uint64_t o0 = rlx_load64(r64 + 3), o1 = rlx_load64(r64 + 4);
    orig.src_ip = (uint32_t)o0; orig.dst_ip = (uint32_t)(o0 >> 32);
    orig.src_port = (uint16_t)o1; orig.dst_port = (uint16_t)(o1 >> 16);
    orig.protocol = (uint8_t)(o1 >> 32);
  }
  uint64_t osig = bng_tuple_sig(orig.src_ip, orig.dst_ip, orig.src_port,
                                orig.dst_port, orig.protocol);
  bng_nat_session* sess = sig_lookup(T.sessions, T.sess_mask, osig);
  if (!sess || !bng_wait_ready(&sess->ready, 8192) ||
      !tuple_eq(sess->key, orig)) {
    /* session expired: clean the reverse entry (ref :871-875) */
    __hip_atomic_store(&rev->sig, BNG_KEY_TOMBSTONE, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    F.sess_expired = true;
    return BNG_FWD;
  }
  (void)0;
  {
    const uint64_t* e64 = (const uint64_t*)sess;
    if (rlx_load64(e64 + 5) != T.now_ns)
      rlx_store64((void*)((uint64_t*)sess + 5), T.now_ns);
    atomicAdd((unsigned long long*)((uint64_t*)sess + 12),
              ((unsigned long long)c.len << 24) | 1ull);
  }
  if (c.proto == 6) {
    if (c.tcp_flags & 0x05)
      sess->state = BNG_NAT_CLOSING;
    else if (sess->state == BNG_NAT_NEW && (c.tcp_flags & 0x10))
      sess->state = BNG_NAT_ESTABLISHED;
  }

  uint32_t old_ip = c.daddr, new_ip = sess->orig_ip;
  st_u32be(p + c.ip_off + 16, new_ip);
  uint16_t ipck = ld_u16be(p + c.ip_off + 10);
  st_u16be(p + c.ip_off + 10, csum_upd32(ipck, old_ip, new_ip));
  uint16_t new_port = sess->orig_port;   /* host-read value at egress */
  if (c.proto == 6) {
    uint16_t old_port = ld_u16be(p + c.l4_off + 2);
    st_u16be(p + c.l4_off + 2, new_port);
    uint16_t ck = ld_u16be(p + c.l4_off + 16);
    ck = csum_upd32(ck, old_ip, new_ip);
    ck = csum_upd16(ck, old_port, new_port);
    st_u16be(p + c.l4_off + 16, ck);
  } else if (c.proto == 17) {
    uint16_t old_port = ld_u16be(p + c.l4_off + 2);
    st_u16be(p + c.l4_off + 2, new_port);
    uint16_t ck = ld_u16be(p + c.l4_off + 6);
    if (ck != 0) {
      ck = csum_upd32(ck, old_ip, new_ip);
      ck = csum_upd16(ck, old_port, new_port);
      if (ck == 0) ck = 0xFFFF;
      st_u16be(p + c.l4_off + 6, ck);
    }
  } else if (c.proto == 1) {
    uint16_t old_id = ld_u16be(p + c.l4_off + 4);
    st_u16be(p + c.l4_off + 4, new_port);
    uint16_t ck = ld_u16be(p + c.l4_off + 2);
    st_u16be(p + c.l4_off + 2, csum_upd16(ck, old_id, new_port));
  }
  F.dnat = true;
  return BNG_FWD;
}

BNG_DEV void nat_count_stats(const nat_flags& F, unsigned long long* sb) {
  sb_fold(sb, SB_NAT + BNG_NS_SNAT, wave_count(F.snat));
  sb_fold(sb, SB_NAT + BNG_NS_DNAT, wave_count(F.dnat));
  sb_fold(sb, SB_NAT + BNG_NS_HAIRPIN, wave_count(F.hairpin));
  sb_fold(sb, SB_NAT + BNG_NS_DROPPED, wave_count(F.dropped));
  sb_fold(sb, SB_NAT + BNG_NS_PASSED, wave_count(F.passed));
  sb_fold(sb, SB_NAT + BNG_NS_SESS_CREATED, wave_count(F.sess_created));
  sb_fold(sb, SB_NAT + BNG_NS_SESS_EXPIRED, wave_count(F.sess_expired));
  sb_fold(sb, SB_NAT + BNG_NS_PORT_EXHAUSTION, wave_count(F.port_exh));
  sb_fold(sb, SB_NAT + BNG_NS_EIM_HITS, wave_count(F.eim_hit));
  sb_fold(sb, SB_NAT + BNG_NS_EIM_MISSES, wave_count(F.eim_miss));
  sb_fold(sb, SB_NAT + BNG_NS_ALG_TRIGGERS, wave_count(F.alg));
  sb_fold(sb, SB_NAT + BNG_NS_ICMP_ERR_XLATE, wave_count(F.icmp_xlate));
  sb_fold(sb, SB_NAT + BNG_NS_ICMP_ERR_NOMAP, wave_count(F.icmp_nomap));
}

/* the bound keeps the 5 waves per SIMD the kernel had before the out-of-line
 * ICMP-error call: values that live across a call sit in the callee-saved
 * ranges, which spreads the allocation to 102 VGPRs without it, 96 with */
__global__ __launch_bounds__(256, 5) void nat44_kernel(
    uint8_t* __restrict__ data, const uint16_t* __restrict__ in_len,
    uint8_t* __restrict__ verdict, int n, int stride, int is_egress,
    bng_nat_session* sessions, uint32_t sess_mask,
    bng_nat_reverse* reverse, uint32_t rev_mask,
    bng_eim_entry* eim, uint32_t eim_mask,
    bng_subctx* ctx, uint32_t ctx_mask,
    const bng_nat_config* cfg,
    const uint32_t* hairpin_ips, uint32_t n_hairpin,
    unsigned long long* stats,
    bng_nat_log_entry* log_ring, bng_ring_header* log_hdr,
    uint64_t now_ns) {
  nat_tables T{sessions, sess_mask, reverse, rev_mask, eim, eim_mask,
               ctx, ctx_mask, cfg, hairpin_ips, n_hairpin, stats,
               log_ring, log_hdr, now_ns};
  __shared__ unsigned long long sb[SB_N];
  sb_zero(sb, SB_N);
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int base = 0; base < n; base += nthreads) {
    int pid = base + tid;
    nat_flags F; F.clear();
    if (pid < n) {
      pktctx c;
      parse_pkt(c, data + (size_t)pid * stride, in_len[pid], false);
      int v = is_egress ? nat_egress_process(c, T, F)
                        : nat_ingress_process(c, T, F);
      verdict[pid] = (uint8_t)v;
    }
    nat_count_stats(F, sb);
  }
  __syncthreads();
  sb_commit(sb, SB_NAT, BNG_NAT_NSTATS, stats);
}

/* ============================================================ QoS  K3 */

struct qos_flags { bool passed, dropped; uint32_t bytes; };

/* byte sums keep a wave reduction (bytes is a frame length, <= 65535 per
 * lane) and accumulate in 64 bits */
BNG_DEV void qos_count_stats(const qos_flags& F, unsigned long long* sb) {
  uint32_t np = wave_count(F.passed), nd = wave_count(F.dropped);
  sb_fold(sb, SB_QOS + BNG_QS_PKT_PASSED, np);
  sb_fold(sb, SB_QOS + BNG_QS_PKT_DROPPED, nd);
  /* wave-uniform branches: every lane takes the reduction or none */
  if (np) sb_fold(sb, SB_QOS + BNG_QS_BYTES_PASSED,
                  wave_sum32(F.passed ? F.bytes : 0u));
  if (nd) sb_fold(sb, SB_QOS + BNG_QS_BYTES_DROPPED,
                  wave_sum32(F.dropped ? F.bytes : 0u));
}

/* Token-bucket check (ref token_bucket_check qos_ratelimit.c:70-104),
 * consume-first form: one atomicAdd(-len) when tokens suffice (the
 * common case); only an INSUFFICIENT balance triggers the refill
 * (elapsed-credit since last_update, capped at burst, refill winner by
 * CAS on last_update) and one retry.  Verdict-equivalent to the
 * reference's refill-then-consume: unclaimed credit stays recoverable
 * because last_update only advances when a refill actually runs. */
BNG_DEV bool qos_consume(int64_t* tokens, uint32_t pkt_len) {
  long long old = (long long)atomicAdd(
      (unsigned long long*)tokens,
      (unsigned long long)(-(int64_t)pkt_len));
  if (old - (int64_t)pkt_len >= 0) return true;
  atomicAdd((unsigned long long*)tokens, (unsigned long long)pkt_len);
  return false;
}

/* Refill credit min(floor(elapsed_ns * bytes_per_s / 1e9), cap), exact for
 * every pair of 64-bit operands.  The product is taken in 128 bits and
 * divided by long division in 32-bit digits: with hi < 1e9 every partial
 * dividend is below 1e9 * 2^32 < 2^62.  A 64-bit product wraps from
 * 14.76 s of idle time at 10 Gbps on.  cap fits 32 bits, so a quotient
 * with a digit above the lowest is the cap.  Runs on the refill path only,
 * which a packet reaches when its first consume failed. */
BNG_DEV uint64_t qos_credit(uint64_t elapsed_ns, uint64_t bytes_per_s,
                            uint32_t cap) {
  const uint64_t D = 1000000000ull;
  uint64_t hi = __umul64hi(elapsed_ns, bytes_per_s);
  uint64_t lo = elapsed_ns * bytes_per_s;
  if (hi >= D) return cap;               /* quotient >= 2^64 */
  uint64_t d1 = (hi << 32) | (lo >> 32);
  uint64_t q1 = d1 / D;
  uint64_t d0 = ((d1 - q1 * D) << 32) | (lo & 0xFFFFFFFFull);
  uint64_t q0 = d0 / D;                  /* d0 < 1e9 * 2^32: q0 < 2^32 */
  return (q1 != 0 || q0 > cap) ? cap : q0;
}

/* field-pointer form so the standalone egress bucket (bng_qos_bucket)
 * and the merged uplink context (bng_subctx) share one implementation.
 * Only a clock that moved forward refills: with now_ns <= last_update (a
 * wall clock stepped back) there is no credit and the stamp stays, so
 * credit resumes once the clock has caught up with it. */
BNG_DEV bool qos_tb_check(int64_t* tokens, uint64_t* last_update,
                          uint32_t burst_bytes, uint32_t pkt_len,
                          uint64_t now_ns, uint64_t rate) {
  if (rate == 0) return true;
  if (qos_consume(tokens, pkt_len)) return true;
  /* insufficient: claim the refill, credit elapsed time, retry once */
  uint64_t last = __hip_atomic_load(last_update, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
  if (last < now_ns &&
      __hip_atomic_compare_exchange_strong(
          last_update, &last, now_ns, __ATOMIC_RELAXED,
          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
    int64_t burst = (int64_t)burst_bytes;
    /* clamped to the burst while still unsigned: the cast cannot wrap */
    uint64_t add = qos_credit(now_ns - last, rate / 8, burst_bytes);
    /* capped add, bounded CAS loop */
    for (int t = 0; t < 16; ++t) {
      int64_t cur = (int64_t)__hip_atomic_load(
          (uint64_t*)tokens, __ATOMIC_RELAXED,
          __HIP_MEMORY_SCOPE_AGENT);
      int64_t want = cur + (int64_t)add;
      if (want > burst) want = burst;
      if (want == cur) break;
      uint64_t expect = (uint64_t)cur;
      if (__hip_atomic_compare_exchange_strong(
              (uint64_t*)tokens, &expect, (uint64_t)want,
              __ATOMIC_RELAXED, __ATOMIC_RELAXED,
              __HIP_MEMORY_SCOPE_AGENT))
        break;
    }
  }
  return qos_consume(tokens, pkt_len);
}

BNG_DEV int qos_process(pktctx& c, bng_qos_bucket* table, uint32_t mask,
                        bool egress, uint64_t now_ns, qos_flags& F) {
  if (c.ip_off < 0) return BNG_FWD;
  uint32_t key = egress ? c.daddr : c.saddr;
  /* table keys are stored as the BE byte pattern read as host int */
  uint64_t rate = 0;
  bng_qos_bucket* tb = qos_lookup(table, mask, key, &rate);
  if (!tb) return BNG_FWD;
  bool ok = qos_tb_check(&tb->tokens, &tb->last_update, tb->burst_bytes,
                         c.len, now_ns, rate);
  F.bytes = c.len;
  if (ok) { F.passed = true; return BNG_FWD; }
  F.dropped = true;
  return BNG_DROP;
}

/* ingress QoS over the merged subscriber context — shares the entry the
 * NAT stage already probed, so the policy check costs no extra walk */
BNG_DEV int qos_process_ctx(pktctx& c, bng_subctx* e, bool qos_valid,
                            uint64_t rate_bps, uint32_t burst_bytes,
                            uint64_t now_ns, qos_flags& F) {
  if (c.ip_off < 0 || !e || !qos_valid) return BNG_FWD;
  bool ok = qos_tb_check(&e->tokens, &e->last_update, burst_bytes, c.len,
                         now_ns, rate_bps);
  F.bytes = c.len;
  if (ok) { F.passed = true; return BNG_FWD; }
  F.dropped = true;
  return BNG_DROP;
}

__global__ void qos_kernel(
    uint8_t* __restrict__ data, const uint16_t* __restrict__ in_len,
    uint8_t* __restrict__ verdict, int n, int stride, int is_egress,
    void* table, uint32_t mask,
    unsigned long long* stats, uint64_t now_ns) {
  __shared__ unsigned long long sb[SB_N];
  sb_zero(sb, SB_N);
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int base = 0; base < n; base += nthreads) {
    int pid = base + tid;
    qos_flags F{false, false, 0};
    if (pid < n) {
      pktctx c;
      parse_pkt(c, data + (size_t)pid * stride, in_len[pid], false);
      int v;
      if (is_egress) {
        v = qos_process(c, (bng_qos_bucket*)table, mask, true, now_ns, F);
      } else {
        /* this kernel goes through the entry once, right here: plain
         * loads, the second one is served by L1 */
        ctx_hit h = subctx_lookup((bng_subctx*)table, mask,
                                  c.ip_off >= 0 ? c.saddr : 0,
                                  /*want_qos=*/false);
        if (h.e && h.qos_valid) {
          h.rate_bps = h.e->rate_bps; h.burst_bytes = h.e->burst_bytes;
        }
        v = qos_process_ctx(c, h.e, h.qos_valid, h.rate_bps, h.burst_bytes,
                            now_ns, F);
      }
      verdict[pid] = (uint8_t)v;
    }
    qos_count_stats(F, sb);
  }
  __syncthreads();
  sb_commit(sb, SB_QOS, BNG_QOS_NSTATS, stats);
}

/* ====================================================== antispoof  K4 */

struct as_flags { bool allowed, dropped, logged, v4viol, v6viol; };

BNG_DEV void as_count_stats(const as_flags& F, unsigned long long* sb) {
  sb_fold(sb, SB_AS + BNG_AS_ALLOWED, wave_count(F.allowed));
  sb_fold(sb, SB_AS + BNG_AS_DROPPED, wave_count(F.dropped));
  sb_fold(sb, SB_AS + BNG_AS_LOGGED, wave_count(F.logged));
  sb_fold(sb, SB_AS + BNG_AS_V4_VIOLATIONS, wave_count(F.v4viol));
  sb_fold(sb, SB_AS + BNG_AS_V6_VIOLATIONS, wave_count(F.v6viol));
}

/* `mac` is the source MAC as the lookup key holds it: byte 0 in bits
 * 40..47 */
BNG_DEV void spoof_log_push(bng_spoof_event* ring, bng_ring_header* hdr,
                            uint64_t mac, uint8_t proto,
                            uint32_t spoofed, uint32_t allowed,
                            uint64_t now_ns) {
  if (!ring) return;
  uint32_t idx = ring_claim(hdr);
  bng_spoof_event* e = &ring[idx & ((1u << BNG_SPOOF_RING_LOG2) - 1)];
  e->timestamp = now_ns;
  #pragma unroll
  for (int i = 0; i < 6; ++i) e->src_mac[i] = (uint8_t)(mac >> (40 - 8 * i));
  e->protocol = proto;
  e->spoofed_ip = spoofed; e->allowed_ip = allowed;
  #pragma unroll
  for (int i = 0; i < 16; ++i) { e->spoofed_ipv6[i] = 0; e->allowed_ipv6[i] = 0; }
}

/* uRPF source validation (ref antispoof_ingress antispoof.c:189-293),
 * quirks preserved (see golden.py docstring).  `proto` is the ethertype,
 * `src_ip` the IPv4 source (read only when proto is 0x0800 and the frame
 * holds it), `smac` the source MAC; binding fields come by value from the
 * probe.  Only the IPv6 source compare reads the frame and the entry. */
BNG_DEV int antispoof_decide(const uint8_t* p, int len, uint32_t proto,
                             uint32_t src_ip, uint64_t smac,
                             const bind_hit& b,
                             const bng_antispoof_config* cfg,
                             bng_spoof_event* ring, bng_ring_header* hdr,
                             uint64_t now_ns, as_flags& F) {
  uint8_t mode = b.e ? b.mode : cfg->default_mode;
  if (mode == BNG_AS_DISABLED) { F.allowed = true; return BNG_FWD; }
  if (proto == 0x0800) {
    if (len < 34) return BNG_FWD;
    bool allowed = false;
    uint32_t bound_ip = 0;
    if (b.e && b.ipv4_valid) {
      bound_ip = b.ipv4_addr;
      if (mode == BNG_AS_STRICT || mode == BNG_AS_LOG_ONLY)
        allowed = (src_ip == bound_ip);
    } else if (mode == BNG_AS_LOOSE) {
      allowed = ip_in_intervals(cfg->allowed_lo, cfg->allowed_hi,
                                cfg->n_allowed_ranges, src_ip);
    }
    if (!allowed) {
      if (cfg->log_violations) {
        spoof_log_push(ring, hdr, smac, 4, src_ip, bound_ip, now_ns);
        F.logged = true;
      }
      if (mode == BNG_AS_LOG_ONLY) { F.allowed = true; return BNG_FWD; }
      F.dropped = true; F.v4viol = true;
      return BNG_DROP;
    }
    F.allowed = true; return BNG_FWD;
  }
  if (proto == 0x86DD) {
    if (len < 14 + 40) return BNG_FWD;
    bool allowed = false;
    if (b.e && b.ipv6_valid) {
      allowed = true;
      #pragma unroll
      for (int i = 0; i < 16; ++i)
        if (p[14 + 8 + i] != b.e->ipv6_addr[i]) { allowed = false; break; }
    } else if (mode == BNG_AS_LOOSE) {
      allowed = true;
    }
    if (!allowed && mode != BNG_AS_LOG_ONLY) {
      if (cfg->log_violations) {
        spoof_log_push(ring, hdr, smac, 6, 0, 0, now_ns);
        F.logged = true;
      }
      F.dropped = true; F.v6viol = true;
      return BNG_DROP;
    }
    F.allowed = true; return BNG_FWD;
  }
  F.allowed = true;
  return BNG_FWD;
}

/* pointer form: ethertype and source address read from the frame (slow
 * path of the fused kernel, stand-alone kernel) */
BNG_DEV int antispoof_process_with(const uint8_t* p, int len, uint64_t smac,
                                   const bind_hit& b,
                                   const bng_antispoof_config* cfg,
                                   bng_spoof_event* ring, bng_ring_header* hdr,
                                   uint64_t now_ns, as_flags& F) {
  uint32_t proto = ld_u16be(p + 12);
  uint32_t src_ip = (proto == 0x0800 && len >= 34) ? ld_u32be(p + 26) : 0;
  return antispoof_decide(p, len, proto, src_ip, smac, b, cfg, ring, hdr,
                          now_ns, F);
}

/* register-window form, for frames the fast parse took (c.regs): untagged
 * IPv4, ihl 5, len >= 48.  Nothing is read from the frame. */
BNG_DEV int antispoof_process_with(const pktctx& c, uint64_t smac,
                                   const bind_hit& b,
                                   const bng_antispoof_config* cfg,
                                   bng_spoof_event* ring, bng_ring_header* hdr,
                                   uint64_t now_ns, as_flags& F) {
  return antispoof_decide(c.p, c.len, 0x0800, c.saddr, smac, b, cfg, ring,
                          hdr, now_ns, F);
}

BNG_DEV int antispoof_process(uint8_t* p, int len,
                              const bng_binding_entry* bindings,
                              uint32_t bmask,
                              const bng_antispoof_config* cfg,
                              bng_spoof_event* ring, bng_ring_header* hdr,
                              uint64_t now_ns, as_flags& F) {
  if (len < 14) return BNG_FWD;
  uint64_t mac = 0;
  #pragma unroll
  for (int i = 0; i < 6; ++i) mac = (mac << 8) | p[6 + i];
  bind_hit b = binding_lookup(bindings, bmask, mac);
  return antispoof_process_with(p, len, mac, b, cfg, ring, hdr, now_ns, F);
}

__global__ void antispoof_kernel(
    uint8_t* __restrict__ data, const uint16_t* __restrict__ in_len,
    uint8_t* __restrict__ verdict, int n, int stride,
    const bng_binding_entry* bindings, uint32_t bmask,
    const bng_antispoof_config* cfg,
    unsigned long long* stats,
    bng_spoof_event* ring, bng_ring_header* hdr, uint64_t now_ns) {
  __shared__ unsigned long long sb[SB_N];
  sb_zero(sb, SB_N);
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int base = 0; base < n; base += nthreads) {
    int pid = base + tid;
    as_flags F{false, false, false, false, false};
    if (pid < n) {
      verdict[pid] = (uint8_t)antispoof_process(
          data + (size_t)pid * stride, in_len[pid], bindings, bmask, cfg,
          ring, hdr, now_ns, F);
    }
    as_count_stats(F, sb);
  }
  __syncthreads();
  sb_commit(sb, SB_AS, BNG_AS_NSTATS, stats);
}

/* ============================== fused uplink pipeline (the hot chain) */
/* One pass per packet over the chain the reference runs as four separate
 * kernel hooks: DHCP fast path for UDP:67, else antispoof -> NAT44 SNAT
 * -> QoS ingress.  One parse, one packet-data round trip — the fusion the
 * CDNA4 guide prescribes for HBM-bound pipelines.
 *
 * Access rule: one burst per line, no plain re-reads.  A line read again
 * after the table probes has left L1 and is fetched from memory a second
 * time, so each line gives up everything the packet needs the first time
 * it is touched:
 *   packet   bytes 0..47 into the register window; the ethertype
 *            pre-check, the MAC, the antispoof stage and the spoof log
 *            read the window.  Only the TCP checksum at byte 50, the IPv6
 *            source and the DHCP body are further loads.
 *   binding  the matching 16-B probe carries address, validity and mode
 *            by value; only the IPv6 compare returns to the entry.
 *   context  the matching probe carries the validity flags, rate and
 *            burst follow at once (L1-bypassing); afterwards the entry
 *            sees atomics only (tokens, refill claim, session create).
 *   session  relaxed agent-scope loads of the hit path, unchanged.
 * Measured: 6.96 M -> 5.13 M memory-side reads per 1M-packet dispatch
 * (profiles/EA_BUDGET.md).
 *
 * Register budget: the default grid (512 blocks of 4 waves on 256 CUs)
 * keeps two waves per SIMD resident, so the bound asks for no more than
 * that.  A tighter cap (5 waves, 96 VGPRs) bought no occupancy the grid
 * ever used and forced 35 VGPR spills into the per-packet loop, whose
 * scratch traffic shares the memory pipe with the table probes. */
__global__ __launch_bounds__(256, 2)
void uplink_pipeline_kernel(bng_uplink_params P) {
  if (P.now_ptr) { P.now_ns = P.now_ptr[0]; P.now_sec = P.now_ptr[1]; }
  dhcp_tables DT{P.subs, P.sub_mask, P.pools, P.n_pools, P.scfg,
                 P.dhcp_stats, P.now_sec};
  nat_tables NT{P.sessions, P.sess_mask, P.reverse, P.rev_mask, P.eim,
                P.eim_mask, P.subctx, P.subctx_mask, P.ncfg, P.hairpin_ips,
                P.n_hairpin, P.nat_stats, P.log_ring, P.log_hdr, P.now_ns};
  __shared__ unsigned long long sb[SB_N];
  sb_zero(sb, SB_N);
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  /* No lane leaves an iteration early: the per-packet body is a
   * do { } while (0) whose `break`s (bad order entry, PPPoE/ARP pass)
   * rejoin the wave BEFORE the wave-wide stat count that ends the
   * iteration, and every thread reaches the barrier after the loop. */
  for (int base = 0; base < P.n; base += nthreads) {
    int i = base + tid;
    dhcp_flags DF; DF.clear();
    nat_flags NF; NF.clear();
    as_flags AF{false, false, false, false, false};
    qos_flags QF{false, false, 0};
    /* with a type-sorted order array, a wave's 64 packets share one
     * code path — divergence between the DHCP and data pipelines no
     * longer serializes both per wave */
    if (i < P.n) do {
      int pid = P.order ? P.order[i] : i;
      if ((unsigned)pid >= (unsigned)P.n) break;  /* defensive */
      uint8_t* p = P.data + (size_t)pid * P.stride;
      int len = P.in_len[pid];
      uint16_t ol = (uint16_t)len;
      int v;
      pktctx c;
      /* PPPoE control/session ethertypes go to the host PPPoE server:
       * the reference's TC_ACT_OK continues the kernel stack where
       * AF_PACKET PPPoE sockets receive them — our FWD would hairpin
       * them back out the wire instead, so the pump equivalent of
       * "continue the stack" is PASS (cli _frame_slow_path). */
      const bool win = pkt_window_load(c, p, len);
      uint16_t et = win ? rg_ld16(c, 12)
          : len >= 14 ? (uint16_t)((p[12] << 8) | p[13]) : 0;
      if (et == 0x8863 || et == 0x8864 || et == 0x0806) {
        P.verdict[pid] = (uint8_t)BNG_PASS;
        P.out_len[pid] = ol;
        break;
      }
      bool ip_ok = (win && parse_pkt_window(c, p, len)) ||
                   parse_pkt_slow(c, p, len, /*want_vlan=*/true);
      bool is_dhcp = ip_ok && c.ip_off >= 0 && c.proto == 17 && c.l4_ok &&
                     c.dport == 67;
      if (is_dhcp) {
        v = dhcp_process_ctx(c, true, P.stride, DT, DF, &ol);
      } else if (ip_ok && !c.tagged && len >= 14) {
        /* hot data path: the two independent first-probe loads
         * (binding / merged subscriber context) issue together; the
         * context entry then serves BOTH the NAT port-block and the
         * ingress-QoS stages — one random HBM touch where the
         * reference's hook chain pays two */
        uint64_t mac;
        if (c.regs) {
          mac = ((uint64_t)rg_ld16(c, 6) << 32) |
                ((uint64_t)rg_ld16(c, 8) << 16) | rg_ld16(c, 10);
        } else {
          mac = 0;
          #pragma unroll
          for (int j = 0; j < 6; ++j) mac = (mac << 8) | p[6 + j];
        }
        uint32_t s0 = (uint32_t)bng_mix64(mac) & P.bmask;
        uint32_t s1 = (uint32_t)bng_mix64(c.saddr) & P.subctx_mask;
        uint4 f0 = ld_probe16(&P.bindings[s0]);
        uint4 f1 = ld_probe16(&P.subctx[s1]);
        bind_hit b = binding_lookup_hint(P.bindings, P.bmask, mac, s0, f0);
        v = c.regs
            ? antispoof_process_with(c, mac, b, P.acfg, P.spoof_ring,
                                     P.spoof_hdr, P.now_ns, AF)
            : antispoof_process_with(p, len, mac, b, P.acfg, P.spoof_ring,
                                     P.spoof_hdr, P.now_ns, AF);
        if (v == BNG_FWD) {
          ctx_hit ctx = subctx_lookup_hint(P.subctx, P.subctx_mask, c.saddr,
                                           s1, f1, /*want_qos=*/true);
          v = nat_egress_ctx(c, NT, NF, ctx.e, ctx.nat_valid);
          if (v == BNG_FWD)
            v = qos_process_ctx(c, ctx.e, ctx.qos_valid, ctx.rate_bps,
                                ctx.burst_bytes, P.now_ns, QF);
        }
      } else {
        /* the reference's TC programs parse untagged frames only
         * (nat44.c:573-581, antispoof.c:194-219): a tagged non-DHCP frame
         * reads as non-IP there and is allowed through */
        v = antispoof_process(p, len, P.bindings, P.bmask, P.acfg,
                              P.spoof_ring, P.spoof_hdr, P.now_ns, AF);
        if (v == BNG_FWD && ip_ok && !c.tagged) {
          ctx_hit ctx = subctx_lookup(P.subctx, P.subctx_mask, c.saddr,
                                      /*want_qos=*/true);
          v = nat_egress_ctx(c, NT, NF, ctx.e, ctx.nat_valid);
          if (v == BNG_FWD)
            v = qos_process_ctx(c, ctx.e, ctx.qos_valid, ctx.rate_bps,
                                ctx.burst_bytes, P.now_ns, QF);
        }
      }
      P.verdict[pid] = (uint8_t)v;
      P.out_len[pid] = ol;
    } while (0);
    dhcp_count_stats(DF, sb);
    nat_count_stats(NF, sb);
    as_count_stats(AF, sb);
    qos_count_stats(QF, sb);
  }
  __syncthreads();
  sb_commit(sb, SB_DHCP, BNG_DHCP_NSTATS, P.dhcp_stats);
  sb_commit(sb, SB_NAT, BNG_NAT_NSTATS, P.nat_stats);
  sb_commit(sb, SB_AS, BNG_AS_NSTATS, P.as_stats);
  sb_commit(sb, SB_QOS, BNG_QOS_NSTATS, P.qos_stats);
}

/* fused downlink pipeline: internet -> subscriber return path.
 * NAT44 DNAT (reverse map -> session -> rewrite) then QoS egress
 * (download shaping keyed by the post-DNAT destination = the
 * subscriber's IP) in one pass — the reference's TC-ingress nat44 +
 * TC-egress qos hook chain (nat44.c:805-948, qos_ratelimit.c:126-172). */
__global__ __launch_bounds__(256, 5)
void downlink_pipeline_kernel(bng_uplink_params P) {
  if (P.now_ptr) { P.now_ns = P.now_ptr[0]; P.now_sec = P.now_ptr[1]; }
  nat_tables NT{P.sessions, P.sess_mask, P.reverse, P.rev_mask, P.eim,
                P.eim_mask, P.subctx, P.subctx_mask, P.ncfg, P.hairpin_ips,
                P.n_hairpin, P.nat_stats, P.log_ring, P.log_hdr, P.now_ns};
  __shared__ unsigned long long sb[SB_N];
  sb_zero(sb, SB_N);
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int base = 0; base < P.n; base += nthreads) {
    int i = base + tid;
    nat_flags NF; NF.clear();
    qos_flags QF{false, false, 0};
    if (i < P.n) {
      int pid = P.order ? P.order[i] : i;
      uint8_t* p = P.data + (size_t)pid * P.stride;
      int len = P.in_len[pid];
      pktctx c;
      bool ip_ok = parse_pkt(c, p, len, false);
      int v = BNG_FWD;
      if (ip_ok) {
        v = nat_ingress_process(c, NT, NF);
        if (v == BNG_FWD && c.ip_off >= 0) {
          /* re-read the (possibly rewritten) destination for QoS */
          c.daddr = ld_u32be(p + c.ip_off + 16);
          v = qos_process(c, P.qos_eg, P.qos_eg_mask, /*egress=*/true,
                          P.now_ns, QF);
        }
      }
      P.verdict[pid] = (uint8_t)v;
      P.out_len[pid] = (uint16_t)len;
    }
    nat_count_stats(NF, sb);
    qos_count_stats(QF, sb);
  }
  __syncthreads();
  sb_commit(sb, SB_NAT, BNG_NAT_NSTATS, P.nat_stats);
  sb_commit(sb, SB_QOS, BNG_QOS_NSTATS, P.qos_stats);
}

/* Class of a frame for type-sorting: 1 = DHCP (IPv4 UDP to port 67, first
 * fragment), 0 = other — for every frame the class that parse_pkt(...,
 * want_vlan=true) and the fused kernel's is_dhcp test give, without
 * running the parser.  The common frame (untagged, ihl 5, row 8-B aligned)
 * is decided from three L1-bypassing 8-B words: ethertype and version/ihl
 * at 12..14, fragment bits and protocol at 20..23, destination port at
 * 36..37.  Tagged frames, IP options and unaligned rows walk the headers
 * byte by byte, bypassing too.  A frame too short to hold the UDP header
 * is class 0, which also keeps every read below `len`. */
BNG_DEV int pkt_classify(const uint8_t* p, int len) {
  if (len >= 42 && !((uintptr_t)p & 7)) {
    uint64_t w1 = rlx_load64(p + 8), w2 = rlx_load64(p + 16);
    uint64_t w4 = rlx_load64(p + 32);
    /* bytes 12, 13, 14 of the frame: ethertype 0x0800, version/ihl 0x45 */
    if (((w1 >> 32) & 0xFFFFFFu) == 0x450008u) {
      bool frag = (w2 & 0xFF1F00000000ull) != 0;     /* bytes 20..21 */
      return !frag && (uint8_t)(w2 >> 56) == 17 &&   /* byte 23 */
             ((w4 >> 32) & 0xFFFFu) == 0x4300u;      /* bytes 36..37 */
    }
  }
  if (len < 14) return 0;
  uint32_t proto = (rlx_load8(p + 12) << 8) | rlx_load8(p + 13);
  int off = 14;
  if (proto == 0x8100 || proto == 0x88A8) {
    if (len < off + 4) return 0;
    proto = (rlx_load8(p + off + 2) << 8) | rlx_load8(p + off + 3);
    off += 4;
    if (proto == 0x8100) {
      if (len < off + 4) return 0;
      proto = (rlx_load8(p + off + 2) << 8) | rlx_load8(p + off + 3);
      off += 4;
    }
  }
  if (proto != 0x0800 || len < off + 20) return 0;
  uint32_t vihl = rlx_load8(p + off);
  if ((vihl >> 4) != 4 || (vihl & 0xF) < 5) return 0;
  int l4_off = off + (int)(vihl & 0xF) * 4;
  if (rlx_load8(p + off + 9) != 17 || len < l4_off + 8) return 0;
  if (((rlx_load8(p + off + 6) << 8) | rlx_load8(p + off + 7)) & 0x1FFF)
    return 0;                                        /* non-first fragment */
  return ((rlx_load8(p + l4_off + 2) << 8) | rlx_load8(p + l4_off + 3)) == 67;
}

__global__ void pkt_class_kernel(const uint8_t* __restrict__ data,
                                 const uint16_t* __restrict__ in_len,
                                 uint8_t* __restrict__ cls, int n,
                                 int stride) {
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int pid = tid; pid < n; pid += nthreads)
    cls[pid] = (uint8_t)pkt_classify(data + (size_t)pid * stride,
                                     in_len[pid]);
}

/* ======================================= host CRUD kernels (pkg/ebpf) */
/* Stream-ordered table upserts/deletes: the MI355X analog of BPF map
 * update syscalls (pkg/ebpf/loader.go:349-661).  Launched on the same HIP
 * stream as the dataplane kernels, so every batch sees a consistent table
 * snapshot (BPF map semantics for free). */

/* HA standby promotion: bulk-restore NAT sessions (+ reverse + EIM)
 * from the active's export records, recreating exactly what the egress
 * create path builds (round-1 VERDICT task 3; ref ha/sync.go session
 * replication keeps NAT bindings across failover). */
__global__ void sess_import_kernel(
    bng_nat_session* sess, uint32_t sess_mask,
    bng_nat_reverse* rev, uint32_t rev_mask,
    bng_eim_entry* eim, uint32_t eim_mask,
    const bng_sess_export* batch, int n, int* rc) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bng_sess_export e = batch[i];
  uint64_t sig = bng_tuple_sig(e.src_ip, e.dst_ip, e.src_port, e.dst_port,
                               e.protocol);
  bng_nat_session* s = sig_find_or_claim(sess, sess_mask, sig).e;
  if (!s) { if (rc) rc[i] = 1; return; }
  /* import is authoritative (runs on a quiesced standby): overwrite on
   * found as well as on claim */
  s->key = bng_nat_tuple{e.src_ip, e.dst_ip, e.src_port, e.dst_port,
                         e.protocol, {0, 0, 0}};
  s->nat_ip = e.nat_ip; s->nat_port = e.nat_port;
  s->orig_port = e.src_port; s->orig_ip = e.src_ip;
  s->state = e.state; s->is_hairpin = e.is_hairpin;
  s->last_seen = e.last_seen; s->created = e.created;
  s->packets_out = 0; s->packets_in = 0;
  s->bytes_out = 0; s->bytes_in = 0;
  bng_publish_ready(&s->ready);

  uint64_t rsig = bng_tuple_sig(e.dst_ip, e.nat_ip, e.dst_port,
                                e.nat_port, e.protocol);
  bng_nat_reverse* r = sig_find_or_claim(rev, rev_mask, rsig).e;
  if (r) {
    r->key = bng_nat_tuple{e.dst_ip, e.nat_ip, e.dst_port, e.nat_port,
                           e.protocol, {0, 0, 0}};
    r->orig = s->key;
    bng_publish_ready(&r->ready);
  } else if (rc) {
    rc[i] = 2;
  }

  if (e.flags & 1) {
    uint64_t esig = bng_eim_sig(e.src_ip, e.src_port, e.protocol);
    const auto mr = sig_find_or_claim(eim, eim_mask, esig);
    bng_eim_entry* m = mr.e;
    if (m) {
      m->internal_ip = e.src_ip; m->internal_port = e.src_port;
      m->protocol = e.protocol;
      m->external_ip = e.nat_ip; m->external_port = e.eim_port;
      m->created = e.created; m->last_used = e.last_seen;
      if (mr.claimed) m->ref_count = 1;
      m->flags = 0;
      bng_publish_ready(&m->ready);
    }
  }
}

__global__ void sub_upsert_kernel(bng_sub_entry* t, uint32_t mask,
                                  const bng_sub_entry* batch, int n,
                                  int* rc) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bng_sub_entry e = batch[i];
  bng_sub_entry* s = key_upsert_slot<&bng_sub_entry::key>(t, mask, e.key);
  if (s) {
    s->pool_id = e.pool_id; s->allocated_ip = e.allocated_ip;
    s->lease_expiry = e.lease_expiry; s->vlan_id = e.vlan_id;
    s->client_class = e.client_class; s->flags = e.flags;
  }
  if (rc) rc[i] = s ? 0 : -1;
}

__global__ void sub_delete_kernel(bng_sub_entry* t, uint32_t mask,
                                  const uint64_t* keys, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bng_sub_entry* s = key_find<&bng_sub_entry::key>(t, mask, keys[i]);
  if (s) rlx_store64(&s->key, BNG_KEY_TOMBSTONE);
}

/* Merge-upsert into the subscriber context.  update_mask selects which
 * half changes (BNG_CTX_SET_NAT / SET_QOS / CLR_QOS / CLR_NAT) so the
 * NAT manager and the QoS manager can each own their fields without
 * clobbering the other's — the BPF-map analog of two maps sharing a key.
 * A clear-only mask on an absent key claims nothing and returns 0. */
__global__ void subctx_upsert_kernel(bng_subctx* t, uint32_t mask,
                                     const bng_subctx* batch, int n,
                                     uint32_t um, int* rc) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bng_subctx e = batch[i];
  bool full;
  bng_subctx* s = ipkey_upsert_slot(
      t, mask, e.key_ip, (um & (BNG_CTX_SET_NAT | BNG_CTX_SET_QOS)) != 0,
      &full);
  if (s) {
    if (um & BNG_CTX_SET_NAT) {
      s->public_ip = e.public_ip;
      s->port_start = e.port_start; s->port_end = e.port_end;
      s->next_port = e.next_port; s->subscriber_id = e.subscriber_id;
      s->flags = e.flags; s->nat_valid = 1;
    }
    if (um & BNG_CTX_SET_QOS) {
      s->rate_bps = e.rate_bps; s->tokens = e.tokens;
      s->last_update = e.last_update; s->burst_bytes = e.burst_bytes;
      s->priority = e.priority; s->qos_valid = 1;
    }
    if (um & BNG_CTX_CLR_QOS) s->qos_valid = 0;
    if (um & BNG_CTX_CLR_NAT) s->nat_valid = 0;
  }
  if (rc) rc[i] = full ? -1 : 0;
}

/* Any upsert claims a slot; valid=0 is how a policy is removed. */
__global__ void qos_upsert_kernel(bng_qos_bucket* t, uint32_t mask,
                                  const bng_qos_bucket* batch, int n,
                                  int* rc) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bng_qos_bucket e = batch[i];
  bool full;
  bng_qos_bucket* s = ipkey_upsert_slot(t, mask, e.key_ip, true, &full);
  if (s) {
    s->rate_bps = e.rate_bps; s->tokens = e.tokens;
    s->last_update = e.last_update; s->burst_bytes = e.burst_bytes;
    s->priority = e.priority;
    s->valid = e.valid;
  }
  if (rc) rc[i] = full ? -1 : 0;
}

__global__ void binding_upsert_kernel(bng_binding_entry* t, uint32_t mask,
                                      const bng_binding_entry* batch, int n,
                                      int* rc) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bng_binding_entry e = batch[i];
  bng_binding_entry* s =
      key_upsert_slot<&bng_binding_entry::key_mac>(t, mask, e.key_mac);
  if (s) {
    s->ipv4_addr = e.ipv4_addr; s->ipv4_valid = e.ipv4_valid;
    s->ipv6_valid = e.ipv6_valid; s->mode = e.mode;
    #pragma unroll
    for (int j = 0; j < 16; ++j) s->ipv6_addr[j] = e.ipv6_addr[j];
  }
  if (rc) rc[i] = s ? 0 : -1;
}

__global__ void binding_delete_kernel(bng_binding_entry* t, uint32_t mask,
                                      const uint64_t* keys, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bng_binding_entry* s =
      key_find<&bng_binding_entry::key_mac>(t, mask, keys[i]);
  if (s) rlx_store64(&s->key_mac, BNG_KEY_TOMBSTONE);
}

/* NAT session sweeper: reclaim timed-out sessions (the LRU-map analog,
 * host-triggered; ref relies on BPF LRU eviction).  Walks the table in
 * parallel; each thread owns a contiguous range of slots. */
__global__ void nat_sweep_kernel(bng_nat_session* sessions, uint32_t n_slots,
                                 bng_nat_reverse* reverse, uint32_t rev_mask,
                                 bng_subctx* ctx,
                                 uint32_t ctx_mask,
                                 bng_eim_entry* eim, uint32_t eim_slots,
                                 uint64_t eim_to,
                                 uint64_t now_ns, uint64_t udp_to,
                                 uint64_t tcp_est_to, uint64_t tcp_tr_to,
                                 uint64_t icmp_to,
                                 unsigned long long* stats) {
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  bool any = false;
  for (uint32_t i = tid; i < n_slots; i += nthreads) {
    bng_nat_session* s = &sessions[i];
    uint64_t sig = s->sig;
    if (sig == BNG_KEY_EMPTY || sig == BNG_KEY_TOMBSTONE || !s->ready)
      continue;
    /* fold the hot-path packed accounting deltas ({bytes:40,pkts:24} in
     * _pad2[0/1]) into the u64 counters.  The packing bounds what one
     * session may carry between two sweeps: 2^24 packets per direction
     * (the 2^40 bytes hold 2^24 frames of 65535 B); past that the packet
     * count carries into the byte field. */
    {
      unsigned long long po = atomicExch(
          (unsigned long long*)&s->_pad2[0], 0ull);
      unsigned long long pi = atomicExch(
          (unsigned long long*)&s->_pad2[1], 0ull);
      if (po) {
        s->packets_out += po & 0xFFFFFFull;
        s->bytes_out += po >> 24;
      }
      if (pi) {
        s->packets_in += pi & 0xFFFFFFull;
        s->bytes_in += pi >> 24;
      }
    }
    uint64_t to = udp_to;
    if (s->key.protocol == 6)
      to = (s->state == BNG_NAT_ESTABLISHED) ? tcp_est_to : tcp_tr_to;
    else if (s->key.protocol == 1)
      to = icmp_to;
    /* a session stamped after now_ns (a wall clock stepped back) has
     * been idle for no time at all; the unsigned difference would wrap
     * and expire every flow touched since */
    uint64_t seen = s->last_seen;
    uint64_t idle = now_ns > seen ? now_ns - seen : 0;
    if (idle < to && s->state != BNG_NAT_CLOSING) continue;
    if (s->state == BNG_NAT_CLOSING && idle < tcp_tr_to) continue;
    /* expire: tombstone session + its reverse entry, decrement counters */
    uint64_t rsig = bng_tuple_sig(s->key.dst_ip, s->nat_ip, s->key.dst_port,
                                  s->nat_port, s->key.protocol);
    bng_nat_reverse* rev = sig_lookup(reverse, rev_mask, rsig);
    if (rev)
      __hip_atomic_store(&rev->sig, BNG_KEY_TOMBSTONE, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    bng_subctx* blk = subctx_lookup(ctx, ctx_mask, s->key.src_ip,
                                    /*want_qos=*/false).e;
    if (blk) atomicSub(&blk->sessions_active, 1u);
    s->ready = 0;
    __hip_atomic_store(&s->sig, BNG_KEY_TOMBSTONE, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    any = true;
    stat_inc(&stats[BNG_NS_SESS_EXPIRED], true);
  }
  (void)any;
  /* EIM idle expiry — the LRU-eviction analog for the endpoint-
   * independent mapping table (the reference's eim_table is an LRU
   * map, nat44.c:231-238).  Safe to expire under live sessions: the
   * reverse map demuxes ingress by the full remote endpoint, so only
   * endpoint-independence for FUTURE flows is (correctly) lost. */
  if (eim != nullptr && eim_to != 0) {
    for (uint32_t i = tid; i < eim_slots; i += nthreads) {
      bng_eim_entry* e = &eim[i];
      uint64_t sig = e->sig;
      if (sig == BNG_KEY_EMPTY || sig == BNG_KEY_TOMBSTONE || !e->ready)
        continue;
      uint64_t used = e->last_used;
      if (now_ns <= used || now_ns - used < eim_to)   /* as above */
        continue;
      e->ready = 0;
      __hip_atomic_store(&e->sig, BNG_KEY_TOMBSTONE, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

/* shard-owner computation for multi-GPU steering: owner by subscriber
 * identity — source IP for upstream IPv4, chaddr MAC for DHCP.  Must match
 * bng_amd/parallel/hashring.py owner_of_* bit-for-bit. */
__global__ void shard_owner_kernel(const uint8_t* __restrict__ data,
                                   const uint16_t* __restrict__ in_len,
                                   int32_t* __restrict__ owner,
                                   int n, int stride, int n_shards) {
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int pid = tid; pid < n; pid += nthreads) {
    const uint8_t* p = data + (size_t)pid * stride;
    int len = in_len[pid];
    uint64_t key = 0;
    if (len >= 34 && ld_u16be(p + 12) == 0x0800) {
      if (p[14 + 9] == 17 && len >= 42 && ld_u16be(p + 14 + 20 + 2) == 67 &&
          len >= 42 + 240) {
        /* DHCP: key by chaddr MAC */
        const uint8_t* ch = p + 42 + 28;
        #pragma unroll
        for (int i = 0; i < 6; ++i) key = (key << 8) | ch[i];
      } else {
        key = ld_u32be(p + 14 + 12);   /* source IP */
      }
    } else if (len >= 14) {
      #pragma unroll
      for (int i = 0; i < 6; ++i) key = (key << 8) | p[6 + i];  /* src MAC */
    }
    owner[pid] = (int32_t)(bng_mix64(key) % (uint64_t)n_shards);
  }
}

/* ============================== PPPoE session-data pre-pass / post-pass */
/* PPPoE subscribers reach the fused pipelines through two small kernels
 * of their own instead of a branch inside them: the uplink kernel sits at
 * its 96-VGPR cap and its register-window parse wants the IPv4 header at
 * byte 14 of a 16-B-aligned row, where a PPPoE session frame has it at
 * byte 22.  pppoe_decap_kernel removes the 8 B of PPPoE + PPP header
 * before the uplink kernel runs, pppoe_encap_kernel re-adds them after the
 * downlink kernel.  Neither is launched while no session is provisioned.
 *
 * Rows are 16-B aligned (the extension checks stride % 16 and the base
 * pointer), so both shifts move 16-B words: the 8-B shift makes every
 * destination word the high half of one source word plus the low half of
 * the next, carried in registers.  No load or store leaves the row. */

/* 16 B at byte offset `off` of a row, or zeros when the word would cross
 * the end of the row (those bytes are past the frame, never needed) */
BNG_DEV uint4 row_ld16(const uint8_t* p, int off, int stride) {
  if (off + 16 > stride) return make_uint4(0, 0, 0, 0);
  return *(const uint4*)(p + off);
}

BNG_DEV uint32_t bswap16(uint32_t v) {
  return ((v & 0xFFu) << 8) | ((v >> 8) & 0xFFu);
}

struct pppoe_flags {
  bool dec_ok, ctrl, unknown, mac_bad, malformed, enc_ok, too_big, no_room;
};

BNG_DEV void pppoe_count_stats(const pppoe_flags& F, unsigned long long* sb) {
  sb_fold(sb, BNG_PS_DECAP_OK, wave_count(F.dec_ok));
  sb_fold(sb, BNG_PS_DECAP_CTRL, wave_count(F.ctrl));
  sb_fold(sb, BNG_PS_DECAP_UNKNOWN_SESSION, wave_count(F.unknown));
  sb_fold(sb, BNG_PS_DECAP_MAC_MISMATCH, wave_count(F.mac_bad));
  sb_fold(sb, BNG_PS_DECAP_MALFORMED, wave_count(F.malformed));
  sb_fold(sb, BNG_PS_ENCAP_OK, wave_count(F.enc_ok));
  sb_fold(sb, BNG_PS_ENCAP_TOO_BIG, wave_count(F.too_big));
  sb_fold(sb, BNG_PS_ENCAP_NO_ROOM, wave_count(F.no_room));
}

/* Uplink pre-pass: a 0x8864 frame carrying PPP IPv4 from a provisioned
 * session becomes the untagged IPoE frame with the same IP packet. */
__global__ __launch_bounds__(256)
void pppoe_decap_kernel(uint8_t* data, uint16_t* in_len,
                        uint8_t* __restrict__ state, int n, int stride,
                        const bng_pppoe_sess* __restrict__ sess,
                        unsigned long long* stats) {
  __shared__ unsigned long long sb[BNG_PPPOE_NSTATS];
  sb_zero(sb, BNG_PPPOE_NSTATS);
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int base = 0; base < n; base += nthreads) {
    int pid = base + tid;
    pppoe_flags F{false, false, false, false, false, false, false, false};
    if (pid < n) do {
      uint8_t* p = data + (size_t)pid * stride;
      int len = in_len[pid];
      if (len > stride) len = stride;      /* a row holds no more */
      uint4 h0 = *(const uint4*)p;         /* bytes 0..15  */
      uint8_t st = BNG_PPPOE_NONE;
      if (len < 14 || (h0.w & 0xFFFFu) != 0x6488u) {   /* 88 64 */
        state[pid] = st;
        break;
      }
      uint4 h1 = *(const uint4*)(p + 16);  /* bytes 16..31 */
      int plen = (int)bswap16(h1.x >> 16);
      if (len < 22 || (h0.w >> 16) != 0x0011u ||       /* ver/type, code */
          plen < 2 || 20 + plen > len) {
        F.malformed = true; st = BNG_PPPOE_REJECT;
      } else if ((h1.y & 0xFFFFu) != 0x2100u) {        /* not PPP IPv4 */
        F.ctrl = true; st = BNG_PPPOE_CTRL;
      } else {
        uint32_t sid = bswap16(h1.x & 0xFFFFu);
        uint4 e = ld_probe16(&sess[sid]);
        uint64_t mv = ((uint64_t)e.y << 32) | e.x;
        uint64_t mac =
            ((uint64_t)(__builtin_bswap32(h0.y) & 0xFFFFu) << 32) |
            __builtin_bswap32(h0.z);
        if (!(mv & BNG_PPPOE_VALID)) {
          F.unknown = true; st = BNG_PPPOE_REJECT;
        } else if ((mv & BNG_PPPOE_MAC_MASK) != mac) {
          F.mac_bad = true; st = BNG_PPPOE_REJECT;
        } else if (plen - 2 < 20) {
          F.malformed = true; st = BNG_PPPOE_REJECT;
        } else {
          F.dec_ok = true; st = BNG_PPPOE_DECAP;
          int nlen = 12 + plen;            /* <= len - 8 <= stride - 8 */
          /* new dword 12: ethertype 08 00 + old bytes 22..23 */
          *(uint32_t*)(p + 12) = 0x0008u | (h1.y & 0xFFFF0000u);
          /* new 16-B word at d = old bytes d+8 .. d+23 */
          uint32_t c0 = h1.z, c1 = h1.w;   /* old bytes 24..31 */
          for (int d = 16; d < nlen; d += 16) {
            uint4 v = row_ld16(p, d + 16, stride);
            *(uint4*)(p + d) = make_uint4(c0, c1, v.x, v.y);
            c0 = v.z; c1 = v.w;
          }
          in_len[pid] = (uint16_t)nlen;
        }
      }
      state[pid] = st;
    } while (0);
    pppoe_count_stats(F, sb);
  }
  __syncthreads();
  sb_commit(sb, 0, BNG_PPPOE_NSTATS, stats);
}

/* Downlink post-pass: a forwarded IPv4 frame whose (DNAT-ed) destination
 * belongs to a PPPoE session gets the session header back. */
__global__ __launch_bounds__(256)
void pppoe_encap_kernel(uint8_t* data, uint16_t* in_len, uint8_t* verdict,
                        uint8_t* __restrict__ state, int n, int stride,
                        const bng_pppoe_ip* __restrict__ by_ip,
                        uint32_t ip_mask,
                        const bng_pppoe_sess* __restrict__ sess,
                        const bng_server_config* __restrict__ scfg,
                        unsigned long long* stats) {
  __shared__ unsigned long long sb[BNG_PPPOE_NSTATS];
  sb_zero(sb, BNG_PPPOE_NSTATS);
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int base = 0; base < n; base += nthreads) {
    int pid = base + tid;
    pppoe_flags F{false, false, false, false, false, false, false, false};
    if (pid < n) do {
      uint8_t* p = data + (size_t)pid * stride;
      int len = in_len[pid];
      uint8_t st = BNG_PPPOE_NONE;
      state[pid] = st;
      if (verdict[pid] != BNG_FWD || len < 34 || len > stride) break;
      uint4 h0 = *(const uint4*)p;                     /* bytes 0..15 */
      if ((h0.w & 0xFFFFu) != 0x0008u) break;          /* 08 00 */
      uint4 v1 = *(const uint4*)(p + 16);              /* bytes 16..31 */
      uint4 v2 = row_ld16(p, 32, stride);              /* bytes 32..47 */
      /* destination address, bytes 30..33 */
      uint32_t daddr = __builtin_bswap32((v1.w >> 16) | (v2.x << 16));
      uint64_t key = BNG_PPPOE_IP_KEY(daddr);
      uint32_t slot = (uint32_t)bng_mix64(key) & ip_mask;
      uint64_t sm = 0;
      bool hit = false;
      for (int i = 0; i < BNG_MAX_PROBE; ++i) {
        uint4 e = ld_probe16(&by_ip[(slot + i) & ip_mask]);
        uint64_t k = ((uint64_t)e.y << 32) | e.x;
        if (k == key) { sm = ((uint64_t)e.w << 32) | e.z; hit = true; break; }
        if (k == BNG_KEY_EMPTY) break;
      }
      if (!hit) break;
      uint32_t sid = (uint32_t)(sm >> 48);
      uint4 se = ld_probe16(&sess[sid]);
      if (!(se.y & 0x80000000u)) break;                /* session gone */
      int mru = (int)(se.w & 0xFFFFu);
      if (len - 14 > mru) {
        F.too_big = true; st = BNG_PPPOE_TOO_BIG;
        verdict[pid] = (uint8_t)BNG_PASS;
      } else if (len + 8 > stride) {
        F.no_room = true; st = BNG_PPPOE_NO_ROOM;
        verdict[pid] = (uint8_t)BNG_PASS;
      } else {
        F.enc_ok = true; st = BNG_PPPOE_ENCAP;
        /* new 16-B word at d = old bytes d-8 .. d+7, highest word first:
         * each store lands on a source word that is already in registers */
        int top = (len + 7) & ~15;         /* last word with a frame byte */
        uint4 hi = row_ld16(p, top, stride);
        for (int d = top; d >= 32; d -= 16) {
          uint4 lo = *(const uint4*)(p + d - 16);
          *(uint4*)(p + d) = make_uint4(lo.z, lo.w, hi.x, hi.y);
          hi = lo;
        }
        /* hi = old bytes 16..31.  Word 16: sid, plen, 00 21, old 14..15,
         * then old bytes 16..23 */
        uint32_t plen = (uint32_t)(len - 14 + 2);
        *(uint4*)(p + 16) = make_uint4(
            bswap16(sid) | (bswap16(plen) << 16),
            0x2100u | (h0.w & 0xFFFF0000u), hi.x, hi.y);
        /* word 0: client MAC, server MAC, 88 64, 11 00 */
        uint32_t mhi = (uint32_t)(sm >> 32) & 0xFFFFu;  /* MAC bytes 0..1 */
        uint32_t mlo = (uint32_t)sm;                    /* MAC bytes 2..5 */
        uint32_t cw0 = bswap16(mhi) | (bswap16(mlo >> 16) << 16);
        uint32_t cw1 = bswap16(mlo & 0xFFFFu);
        const uint8_t* sv = scfg->server_mac;
        cw1 |= ((uint32_t)sv[0] << 16) | ((uint32_t)sv[1] << 24);
        uint32_t cw2 = (uint32_t)sv[2] | ((uint32_t)sv[3] << 8) |
                       ((uint32_t)sv[4] << 16) | ((uint32_t)sv[5] << 24);
        *(uint4*)p = make_uint4(cw0, cw1, cw2, 0x00116488u);
        in_len[pid] = (uint16_t)(len + 8);
      }
      state[pid] = st;
    } while (0);
    pppoe_count_stats(F, sb);
  }
  __syncthreads();
  sb_commit(sb, 0, BNG_PPPOE_NSTATS, stats);
}

/* Stream-ordered session CRUD, one thread per batch record, under the
 * batch contract of the host CRUD probes: a batch must not name the same
 * session id or the same IP twice. */
BNG_DEV void pppoe_ip_remove(bng_pppoe_ip* t, uint32_t mask, uint32_t ip,
                             uint32_t sid) {
  bng_pppoe_ip* s =
      key_find<&bng_pppoe_ip::key>(t, mask, BNG_PPPOE_IP_KEY(ip));
  /* only the owner removes it: the address may already belong to a newer
   * session */
  if (s && (uint32_t)(s->sid_mac >> 48) == sid)
    rlx_store64(&s->key, BNG_KEY_TOMBSTONE);
}

__global__ void pppoe_sess_upsert_kernel(bng_pppoe_sess* sess,
                                         bng_pppoe_ip* t, uint32_t mask,
                                         const bng_pppoe_sess* batch, int n,
                                         int* rc) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bng_pppoe_sess e = batch[i];
  uint32_t sid = e.session_id;
  uint64_t mac = e.mac_valid & BNG_PPPOE_MAC_MASK;
  bng_pppoe_sess old = sess[sid];
  /* same id, other address: the stale by-IP entry must go */
  if ((old.mac_valid & BNG_PPPOE_VALID) && old.ip != e.ip)
    pppoe_ip_remove(t, mask, old.ip, sid);
  bng_pppoe_ip* s =
      key_upsert_slot<&bng_pppoe_ip::key>(t, mask, BNG_PPPOE_IP_KEY(e.ip));
  if (!s) {
    /* by-IP chain full: leave the session out of both tables so the two
     * directions stay consistent */
    sess[sid] = bng_pppoe_sess{0, 0, 0, 0};
    if (rc) rc[i] = -1;
    return;
  }
  s->sid_mac = ((uint64_t)sid << 48) | mac;
  e.mac_valid = mac | BNG_PPPOE_VALID;
  sess[sid] = e;
  if (rc) rc[i] = 0;
}

__global__ void pppoe_sess_delete_kernel(bng_pppoe_sess* sess,
                                         bng_pppoe_ip* t, uint32_t mask,
                                         const int32_t* sids, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t sid = (uint32_t)sids[i] & 0xFFFFu;
  bng_pppoe_sess old = sess[sid];
  if (!(old.mac_valid & BNG_PPPOE_VALID)) return;
  pppoe_ip_remove(t, mask, old.ip, sid);
  sess[sid] = bng_pppoe_sess{0, 0, 0, 0};
}

/* ==================================== per-subscriber traffic accounting */
/* Billing counts forwarded bytes and packets per subscriber, so accounting
 * must know the verdict, and on the uplink it must key on the source
 * address that SNAT overwrites.  Like PPPoE it therefore lives in small
 * kernels around the fused pipelines instead of inside them (the uplink
 * kernel has no registers to spare): acct_resolve_kernel ahead of the
 * uplink pipeline turns the source address into a table slot,
 * acct_commit_kernel behind it adds what the verdict says, and
 * acct_downlink_kernel does both behind the downlink pipeline, on the
 * DNAT-rewritten destination.  None is launched while no entry is live.
 *
 * Rows are 16-B aligned (the extension checks), so the frame is read with
 * the 16-B window loads of the PPPoE kernels; the commit reads no packet
 * bytes at all. */

/* Slot of the entry of an untagged IPv4 frame's source (or destination)
 * address, or -1: not IPv4, too short, or nobody accounts that address. */
template <bool BY_DST>
BNG_DEV int acct_resolve(const bng_acct_entry* __restrict__ t, uint32_t mask,
                         const uint8_t* p, int len, int stride) {
  if (len < 34) return -1;
  uint4 h0 = *(const uint4*)p;                       /* bytes 0..15  */
  if ((h0.w & 0xFFFFu) != 0x0008u) return -1;        /* 08 00 */
  uint4 h1 = *(const uint4*)(p + 16);                /* bytes 16..31 */
  uint32_t ip;
  if (BY_DST) {
    uint4 h2 = row_ld16(p, 32, stride);              /* bytes 32..47 */
    ip = __builtin_bswap32((h1.w >> 16) | (h2.x << 16));   /* 30..33 */
  } else {
    ip = __builtin_bswap32((h1.z >> 16) | (h1.w << 16));   /* 26..29 */
  }
  uint64_t key = BNG_ACCT_KEY(ip);
  uint32_t slot = (uint32_t)bng_mix64(key) & mask;
  for (int i = 0; i < BNG_MAX_PROBE; ++i) {
    uint32_t s = (slot + i) & mask;
    uint4 e = ld_probe16(&t[s]);
    uint64_t k = ((uint64_t)e.y << 32) | e.x;
    if (k == key) return (int)s;
    if (k == BNG_KEY_EMPTY) return -1;
  }
  return -1;
}

BNG_DEV void acct_add64(uint64_t* p, uint64_t v) {
  /* result unused: a no-return global atomic */
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

/* One entry's adds: `fwd` forwarded packets of `bytes` in total, `drop`
 * dropped ones.  last_seen needs no max: batches are stream-ordered and
 * every writer of a batch stores the same now_ns. */
template <bool DOWN>
BNG_DEV void acct_issue(bng_acct_entry* e, uint32_t fwd, uint32_t bytes,
                        uint32_t drop, uint64_t now_ns) {
  if (fwd) {
    acct_add64(DOWN ? &e->down_pkts : &e->up_pkts, fwd);
    acct_add64(DOWN ? &e->down_bytes : &e->up_bytes, bytes);
    rlx_store64(&e->last_seen, now_ns);
  }
  if (drop) acct_add64(DOWN ? &e->down_drop_pkts : &e->up_drop_pkts, drop);
}

/* Wave-level commit.  Subscriber traffic is heavy-tailed: one busy
 * subscriber can own most lanes of a wave, and 64 lanes adding to one
 * cache line serialise at the memory side.  So up to `rounds` times the
 * wave peels the group of the first pending lane — all pending lanes with
 * that lane's slot — sums the group and lets its first lane issue the
 * adds.  A round that finds a group of one ends the peeling (the wave then
 * looks like distinct subscribers, where peeling is pure overhead), and
 * whatever is still pending after the rounds goes out as per-lane atomics.
 * rounds = 0: no combining; rounds < 0: peel until nothing is pending.
 * Exact for every distribution of slots over lanes: a lane leaves
 * `pending` only when its group's sum has been issued.
 *
 * Must be reached by every lane of the wave (ballots, readlane, shuffles):
 * lanes with nothing to add pass slot = -1.  `bytes` <= 65535 per lane, so
 * a wave's sum fits 32 bits. */
template <bool DOWN>
BNG_DEV void acct_commit_wave(bng_acct_entry* t, int slot, bool fwd,
                              bool drop, uint32_t bytes, uint64_t now_ns,
                              int rounds) {
  bool pending = slot >= 0 && (fwd || drop);
  if (!fwd) bytes = 0;
  int lane = threadIdx.x & 63;
  for (int r = 0; rounds < 0 || r < rounds; ++r) {
    unsigned long long m = __ballot(pending);
    if (m == 0) break;                       /* wave-uniform */
    int first = __ffsll(m) - 1;
    int gslot = __builtin_amdgcn_readlane(slot, first);
    bool mine = pending && slot == gslot;
    unsigned long long g = __ballot(mine);
    if ((g & (g - 1)) == 0) break;           /* a group of one: stop */
    uint32_t nf = wave_count(mine && fwd);
    uint32_t nd = wave_count(mine && drop);
    uint32_t nb = wave_sum32(mine ? bytes : 0u);
    if (lane == first) acct_issue<DOWN>(&t[gslot], nf, nb, nd, now_ns);
    pending = pending && !mine;
  }
  if (pending)
    acct_issue<DOWN>(&t[slot], fwd ? 1u : 0u, bytes, drop ? 1u : 0u, now_ns);
}

/* Uplink pre-pass: after pppoe_decap, before the pipeline.  slot[] is
 * indexed by packet id, like verdict[], so a sorted dispatch order of the
 * pipeline between the two passes changes nothing. */
__global__ __launch_bounds__(256)
void acct_resolve_kernel(const uint8_t* __restrict__ data,
                         const uint16_t* __restrict__ in_len,
                         int32_t* __restrict__ slot, int n, int stride,
                         const bng_acct_entry* __restrict__ t,
                         uint32_t mask) {
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int pid = tid; pid < n; pid += nthreads)
    slot[pid] = acct_resolve<false>(t, mask, data + (size_t)pid * stride,
                                    in_len[pid], stride);
}

/* Uplink post-pass: after the pipeline and the launcher's PPPoE-reject
 * fill.  Reads slot[], verdict[] and out_len[] only.  FWD is billed, DROP
 * is counted, PASS and TX (a DHCP reply is not subscriber traffic) count
 * nothing.  No lane leaves an iteration early: every lane of a wave
 * reaches acct_commit_wave, lanes past n with slot -1. */
__global__ __launch_bounds__(256)
void acct_commit_kernel(bng_acct_entry* t, uint32_t mask,
                        const int32_t* __restrict__ slot,
                        const uint8_t* __restrict__ verdict,
                        const uint16_t* __restrict__ out_len, int n,
                        uint64_t now_ns, int rounds) {
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int base = 0; base < n; base += nthreads) {
    int pid = base + tid;
    int s = -1;
    bool fwd = false, drop = false;
    uint32_t bytes = 0;
    if (pid < n) do {
      s = slot[pid];
      if ((uint32_t)s > mask) { s = -1; break; }     /* -1, or defensive */
      uint8_t v = verdict[pid];
      fwd = v == BNG_FWD;
      drop = v == BNG_DROP;
      bytes = out_len[pid];
    } while (0);
    acct_commit_wave<false>(t, s, fwd, drop, bytes, now_ns, rounds);
  }
}

/* Downlink post-pass: after the pipeline, before pppoe_encap, so both
 * directions count the IPoE frame length.  Resolves on the DNAT-rewritten
 * destination — a frame NAT dropped for lack of a session still carries
 * the public address, resolves to nothing and is not counted — and commits
 * in the same launch. */
__global__ __launch_bounds__(256)
void acct_downlink_kernel(const uint8_t* __restrict__ data,
                          const uint16_t* __restrict__ in_len,
                          const uint8_t* __restrict__ verdict, int n,
                          int stride, bng_acct_entry* t, uint32_t mask,
                          uint64_t now_ns, int rounds) {
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int base = 0; base < n; base += nthreads) {
    int pid = base + tid;
    int s = -1;
    bool fwd = false, drop = false;
    uint32_t bytes = 0;
    if (pid < n) do {
      uint8_t v = verdict[pid];
      fwd = v == BNG_FWD;
      drop = v == BNG_DROP;
      if (!fwd && !drop) break;
      bytes = in_len[pid];
      s = acct_resolve<true>(t, mask, data + (size_t)pid * stride,
                             (int)bytes, stride);
    } while (0);
    acct_commit_wave<true>(t, s, fwd, drop, bytes, now_ns, rounds);
  }
}

/* Stream-ordered entry CRUD, one thread per batch record, under the batch
 * contract of the host CRUD probes: a batch must not name the same address
 * twice. */
__global__ void acct_upsert_kernel(bng_acct_entry* t, uint32_t mask,
                                   const uint32_t* __restrict__ ips, int n,
                                   int reset, int* rc) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t key = BNG_ACCT_KEY(ips[i]);
  bool existed = key_find<&bng_acct_entry::key>(t, mask, key) != nullptr;
  bng_acct_entry* e = key_upsert_slot<&bng_acct_entry::key>(t, mask, key);
  if (!e) { rc[i] = -1; return; }
  /* a fresh claim may sit on a tombstone that still holds the previous
   * owner's counters */
  if (!existed || reset) {
    e->up_bytes = 0; e->up_pkts = 0; e->down_bytes = 0; e->down_pkts = 0;
    e->up_drop_pkts = 0; e->down_drop_pkts = 0; e->last_seen = 0;
  }
  rc[i] = 0;
}

BNG_DEV void acct_copy_out(bng_acct_entry* out, const bng_acct_entry* e) {
  uint4* o = (uint4*)out;
  const uint4* s = (const uint4*)e;
  uint4 z = make_uint4(0, 0, 0, 0);
  #pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = e ? s[k] : z;   /* absent: key == 0 */
}

__global__ void acct_read_kernel(bng_acct_entry* t, uint32_t mask,
                                 const uint32_t* __restrict__ ips, int n,
                                 bng_acct_entry* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  acct_copy_out(&out[i], key_find<&bng_acct_entry::key>(
      t, mask, BNG_ACCT_KEY(ips[i])));
}

/* The final counters for the Stop record: copy, then tombstone, in one
 * stream-ordered step no packet kernel can fall between. */
__global__ void acct_delete_kernel(bng_acct_entry* t, uint32_t mask,
                                   const uint32_t* __restrict__ ips, int n,
                                   bng_acct_entry* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bng_acct_entry* e =
      key_find<&bng_acct_entry::key>(t, mask, BNG_ACCT_KEY(ips[i]));
  acct_copy_out(&out[i], e);
  if (e) rlx_store64(&e->key, BNG_KEY_TOMBSTONE);
}

/* ================================================== walled-garden gate */
/* A quarantined subscriber has no port block and no QoS policy, so the
 * fused uplink kernel would hand every data frame of theirs to the host,
 * and a blocked subscriber who still holds a port block would keep full
 * service.  The gate decides both on the device, for every untagged IPv4
 * frame, in two small kernels around the pipelines (the uplink kernel has
 * no registers to spare): wg_uplink_kernel ahead of the uplink pipeline,
 * keyed on the source address, takes the frames it decides out of the
 * pipeline's dispatch order; wg_downlink_kernel behind the downlink
 * pipeline, keyed on the DNAT-rewritten destination, turns FWD into DROP.
 * Neither is launched while no garden entry is live.  The decision table
 * is GoldenDataplane.garden_uplink / garden_downlink.
 *
 * Rows are 16-B aligned (the extension checks), so the frame is read with
 * the 16-B window loads of the PPPoE and accounting kernels: the three
 * windows of bytes 0..47, and for a header with IP options the one (or
 * two) that hold the ports.  No packet byte is written. */

/* What the gate needs of a frame.  `eligible`: untagged IPv4, version 4,
 * ihl >= 5, at least 34 B.  `ports`: TCP or UDP, first fragment, and the
 * frame holds the whole TCP (20 B) / UDP (8 B) header; every other frame
 * is portless. */
struct wg_frame {
  bool eligible, ports;
  uint32_t saddr, daddr;      /* host ints of the BE fields */
  uint32_t sport, dport;
  uint32_t proto;
  uint64_t smac;              /* as mac_to_u64 */
};

BNG_DEV wg_frame wg_parse(const uint8_t* p, int len, int stride) {
  wg_frame f{false, false, 0, 0, 0, 0, 0, 0};
  if (len > stride) len = stride;                    /* a row holds no more */
  if (len < 34) return f;
  uint4 h0 = *(const uint4*)p;                       /* bytes 0..15  */
  if ((h0.w & 0xFFFFu) != 0x0008u) return f;         /* 08 00 */
  uint32_t vihl = (h0.w >> 16) & 0xFFu;              /* byte 14 */
  uint32_t ihl = vihl & 0xFu;
  if ((vihl >> 4) != 4u || ihl < 5u) return f;
  uint4 h1 = *(const uint4*)(p + 16);                /* bytes 16..31 */
  uint4 h2 = row_ld16(p, 32, stride);                /* bytes 32..47 */
  f.eligible = true;
  f.smac = ((uint64_t)(__builtin_bswap32(h0.y) & 0xFFFFu) << 32) |
           __builtin_bswap32(h0.z);                  /* bytes 6..11 */
  f.proto = h1.y >> 24;                              /* byte 23 */
  f.saddr = __builtin_bswap32((h1.z >> 16) | (h1.w << 16));   /* 26..29 */
  f.daddr = __builtin_bswap32((h1.w >> 16) | (h2.x << 16));   /* 30..33 */
  bool frag = (bswap16(h1.y & 0xFFFFu) & 0x1FFFu) != 0;       /* 20..21 */
  int l4 = 14 + 4 * (int)ihl;                        /* 34..74 */
  int need = f.proto == 6 ? 20 : 8;
  if ((f.proto != 6 && f.proto != 17) || frag || l4 + need > len) return f;
  /* sport and dport, bytes l4..l4+3.  They are inside the frame, so the
   * 16-B window(s) that hold them are inside the row.  l4 is 2 mod 4: the
   * four bytes straddle two dwords, and two windows when l4 is 14 mod 16.
   * The dword pick is a select chain: indexing the window would put it in
   * scratch memory. */
  int w = l4 & ~15, k = (l4 & 15) >> 2;
  uint4 a = w == 32 ? h2 : row_ld16(p, w, stride);
  uint32_t lo = k == 0 ? a.x : k == 1 ? a.y : k == 2 ? a.z : a.w;
  uint32_t hi;
  if (k == 3) hi = row_ld16(p, w + 16, stride).x;
  else hi = k == 0 ? a.y : k == 1 ? a.z : a.w;
  uint32_t raw = (lo >> 16) | (hi << 16);
  f.sport = bswap16(raw & 0xFFFFu);
  f.dport = bswap16(raw >> 16);
  f.ports = true;
  return f;
}

/* mac_state of the entry of `ip`, or 0: nobody quarantines that address */
BNG_DEV uint64_t wg_lookup(const bng_wg_entry* __restrict__ t, uint32_t mask,
                           uint32_t ip) {
  uint64_t key = BNG_WG_KEY(ip);
  uint32_t slot = (uint32_t)bng_mix64(key) & mask;
  for (int i = 0; i < BNG_MAX_PROBE; ++i) {
    uint4 e = ld_probe16(&t[(slot + i) & mask]);
    uint64_t k = ((uint64_t)e.y << 32) | e.x;
    if (k == key) return ((uint64_t)e.w << 32) | e.z;
    if (k == BNG_KEY_EMPTY) return 0;
  }
  return 0;
}

/* Membership in the sorted allow-list (at most 64 keys, L2-resident):
 * (ip, port, proto) when the frame has readable ports, else the bare
 * address. */
BNG_DEV bool wg_allowed(const bng_wg_config* __restrict__ cfg, bool ports,
                        uint32_t ip, uint32_t port, uint32_t proto) {
  if (ports) {
    uint64_t key = ((uint64_t)ip << 32) | ((uint64_t)port << 16) | proto;
    uint32_t n = cfg->n_allowed;
    int lo = 0, hi = (int)(n < BNG_MAX_WG_ALLOWED ? n : BNG_MAX_WG_ALLOWED);
    while (lo < hi) {
      int mid = (lo + hi) >> 1;
      uint64_t v = cfg->allowed_key[mid];
      if (v == key) return true;
      if (v < key) lo = mid + 1; else hi = mid;
    }
    return false;
  }
  uint32_t n = cfg->n_allowed_ips;
  int lo = 0, hi = (int)(n < BNG_MAX_WG_ALLOWED ? n : BNG_MAX_WG_ALLOWED);
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    uint32_t v = cfg->allowed_ip[mid];
    if (v == ip) return true;
    if (v < ip) lo = mid + 1; else hi = mid;
  }
  return false;
}

BNG_DEV bool wg_redirects(const bng_wg_config* __restrict__ cfg,
                          uint32_t port) {
  uint32_t n = cfg->n_redirect_ports;
  if (n > BNG_MAX_WG_REDIRECT_PORTS) n = BNG_MAX_WG_REDIRECT_PORTS;
  for (uint32_t i = 0; i < n; ++i)
    if (cfg->redirect_port[i] == port) return true;
  return false;
}

/* Uplink pre-pass: after pppoe_decap and acct_resolve, before the
 * pipeline.  Position i handles packet order_in[i] (i without an order) and
 * writes order_out[i]: the packet id, or -1 for a frame the gate decided —
 * the pipeline skips an order entry outside [0, n) before it reads or
 * writes anything, so such a frame never reaches antispoof, NAT or QoS.
 * gate[] is written for every packet, verdict[] and out_len[] only for the
 * decided ones.  No lane leaves an iteration early: every lane reaches the
 * wave-wide stat counts. */
__global__ __launch_bounds__(256)
void wg_uplink_kernel(const uint8_t* __restrict__ data,
                      const uint16_t* __restrict__ in_len,
                      uint8_t* __restrict__ verdict,
                      uint16_t* __restrict__ out_len,
                      uint8_t* __restrict__ gate,
                      const int32_t* __restrict__ order_in,
                      int32_t* __restrict__ order_out, int n, int stride,
                      const bng_wg_entry* __restrict__ table, uint32_t mask,
                      const bng_wg_config* __restrict__ cfg,
                      unsigned long long* stats) {
  __shared__ unsigned long long sb[BNG_WG_NSTATS];
  sb_zero(sb, BNG_WG_NSTATS);
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int base = 0; base < n; base += nthreads) {
    int i = base + tid;
    uint32_t g = BNG_WG_NONE;
    if (i < n) do {
      int pid = order_in ? order_in[i] : i;
      if ((unsigned)pid >= (unsigned)n) {            /* not ours to judge */
        order_out[i] = pid;
        break;
      }
      int len = in_len[pid];
      wg_frame f = wg_parse(data + (size_t)pid * stride, len, stride);
      uint64_t ms = f.eligible ? wg_lookup(table, mask, f.saddr) : 0;
      uint32_t state = (uint32_t)(ms >> BNG_WG_STATE_SHIFT);
      uint8_t v = BNG_DROP;
      if (state == BNG_WG_BLOCKED) {
        g = BNG_WG_DROP_BLOCKED;
      } else if (state != BNG_WG_WALLED) {
        g = BNG_WG_NONE;
      } else if ((ms & BNG_WG_MAC_MASK) != f.smac) {
        g = BNG_WG_DROP_MAC;                         /* the gate's uRPF */
      } else if (f.ports && f.proto == 17 && f.dport == 67) {
        g = BNG_WG_NONE;                             /* a lease renewal */
      } else if (wg_allowed(cfg, f.ports, f.daddr, f.dport, f.proto)) {
        g = BNG_WG_ALLOW; v = BNG_FWD;
      } else if (f.ports && f.proto == 6 && wg_redirects(cfg, f.dport)) {
        g = BNG_WG_REDIRECT; v = BNG_PASS;
      } else {
        g = BNG_WG_DROP_WALLED;
      }
      gate[pid] = (uint8_t)g;
      if (g != BNG_WG_NONE) {
        verdict[pid] = v;
        out_len[pid] = (uint16_t)len;
      }
      order_out[i] = g != BNG_WG_NONE ? -1 : pid;
    } while (0);
    sb_fold(sb, BNG_WS_UP_ALLOWED, wave_count(g == BNG_WG_ALLOW));
    sb_fold(sb, BNG_WS_UP_REDIRECTED, wave_count(g == BNG_WG_REDIRECT));
    sb_fold(sb, BNG_WS_UP_DROP_WALLED, wave_count(g == BNG_WG_DROP_WALLED));
    sb_fold(sb, BNG_WS_UP_DROP_BLOCKED, wave_count(g == BNG_WG_DROP_BLOCKED));
    sb_fold(sb, BNG_WS_UP_DROP_MAC, wave_count(g == BNG_WG_DROP_MAC));
  }
  __syncthreads();
  sb_commit(sb, 0, BNG_WG_NSTATS, stats);
}

/* Downlink post-pass: after the pipeline, before acct_downlink and
 * pppoe_encap.  Only a forwarded, eligible frame whose (DNAT-rewritten)
 * destination is in the garden is judged; the gate can only turn FWD into
 * DROP. */
__global__ __launch_bounds__(256)
void wg_downlink_kernel(const uint8_t* __restrict__ data,
                        const uint16_t* __restrict__ in_len,
                        uint8_t* __restrict__ verdict,
                        uint8_t* __restrict__ gate, int n, int stride,
                        const bng_wg_entry* __restrict__ table,
                        uint32_t mask,
                        const bng_wg_config* __restrict__ cfg,
                        unsigned long long* stats) {
  __shared__ unsigned long long sb[BNG_WG_NSTATS];
  sb_zero(sb, BNG_WG_NSTATS);
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  int nthreads = gridDim.x * blockDim.x;
  for (int base = 0; base < n; base += nthreads) {
    int pid = base + tid;
    uint32_t g = BNG_WG_NONE;
    if (pid < n) do {
      if (verdict[pid] != BNG_FWD) { gate[pid] = BNG_WG_NONE; break; }
      wg_frame f = wg_parse(data + (size_t)pid * stride, in_len[pid],
                            stride);
      uint64_t ms = f.eligible ? wg_lookup(table, mask, f.daddr) : 0;
      uint32_t state = (uint32_t)(ms >> BNG_WG_STATE_SHIFT);
      if (state == BNG_WG_BLOCKED) {
        g = BNG_WG_DROP_BLOCKED;
      } else if (state != BNG_WG_WALLED) {
        g = BNG_WG_NONE;
      } else if (wg_allowed(cfg, f.ports, f.saddr, f.sport, f.proto)) {
        g = BNG_WG_ALLOW;
      } else {
        g = BNG_WG_DROP_WALLED;
      }
      gate[pid] = (uint8_t)g;
      if (g == BNG_WG_DROP_WALLED || g == BNG_WG_DROP_BLOCKED)
        verdict[pid] = (uint8_t)BNG_DROP;
    } while (0);
    sb_fold(sb, BNG_WS_DOWN_ALLOWED, wave_count(g == BNG_WG_ALLOW));
    sb_fold(sb, BNG_WS_DOWN_DROP_WALLED,
            wave_count(g == BNG_WG_DROP_WALLED));
    sb_fold(sb, BNG_WS_DOWN_DROP_BLOCKED,
            wave_count(g == BNG_WG_DROP_BLOCKED));
  }
  __syncthreads();
  sb_commit(sb, 0, BNG_WG_NSTATS, stats);
}

/* Stream-ordered entry CRUD, one thread per batch record, under the batch
 * contract of the host CRUD probes: a batch must not name the same address
 * twice.  An upsert of a live address replaces its MAC and state in place;
 * the batch records carry the key already (BNG_WG_KEY of the address). */
__global__ void wg_upsert_kernel(bng_wg_entry* t, uint32_t mask,
                                 const bng_wg_entry* __restrict__ batch,
                                 int n, int* rc) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bng_wg_entry r = batch[i];
  bng_wg_entry* e = key_upsert_slot<&bng_wg_entry::key>(t, mask, r.key);
  if (!e) { rc[i] = -1; return; }
  rlx_store64(&e->mac_state, r.mac_state);
  rc[i] = 0;
}

__global__ void wg_delete_kernel(bng_wg_entry* t, uint32_t mask,
                                 const uint32_t* __restrict__ ips, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bng_wg_entry* e =
      key_find<&bng_wg_entry::key>(t, mask, BNG_WG_KEY(ips[i]));
  if (e) rlx_store64(&e->key, BNG_KEY_TOMBSTONE);
}

/* ============================= extern "C" launchers for the extension */

/* Grid cap of the six batched packet kernels (grid-stride above it).
 * Stats commit once per block, so fewer, longer-lived blocks mean fewer
 * global atomics.  512 = two co-resident blocks on each of the 256 CUs:
 * a 1M-packet batch is eight even iterations with no tail.  Picked by a
 * sweep on the 1M-packet headline, where it beat every cap from 256 to
 * 4096 (profiles/STATS_ATOMICS.md).  bng_set_pkt_grid_cap() overrides it
 * for A/B runs and lets tests force several loop iterations at tiny n; a
 * captured graph keeps the grid it was captured with. */
#define BNG_PKT_GRID_CAP_DEFAULT 512
static int g_pkt_grid_cap = BNG_PKT_GRID_CAP_DEFAULT;

static inline int pkt_grid(int n) {
  int blocks = (n + 255) / 256;
  return blocks < g_pkt_grid_cap ? blocks : g_pkt_grid_cap;
}

/* Peel rounds of the accounting commit (acct_commit_wave): 0 = per-lane
 * atomics only, < 0 = peel until nothing is pending.  The default is the
 * variant profiles/ACCOUNTING.md picks; bng_set_acct_combine() overrides
 * it for A/B runs and tests. */
#define BNG_ACCT_ROUNDS_DEFAULT 4
static int g_acct_rounds = BNG_ACCT_ROUNDS_DEFAULT;

/* classify / shard-owner helpers keep their own fixed cap */
static inline int aux_grid(int n) {
  int blocks = (n + 255) / 256;
  return blocks < 4096 ? blocks : 4096;
}

extern "C" {

void bng_set_pkt_grid_cap(int blocks) {
  g_pkt_grid_cap = blocks > 0 ? blocks : BNG_PKT_GRID_CAP_DEFAULT;
}
int bng_get_pkt_grid_cap(void) { return g_pkt_grid_cap; }

void bng_launch_dhcp(void* data, const void* in_len, void* out_len,
                     void* verdict, int n, int stride,
                     const void* subs, uint32_t sub_mask,
                     const void* pools, uint32_t n_pools, const void* cfg,
                     void* stats, uint64_t now_sec, const void* now_ptr,
                     hipStream_t s) {
  hipLaunchKernelGGL(dhcp_fastpath_kernel, dim3(pkt_grid(n)), dim3(256), 0, s,
      (uint8_t*)data, (const uint16_t*)in_len, (uint16_t*)out_len,
      (uint8_t*)verdict, n, stride, (const bng_sub_entry*)subs, sub_mask,
      (const bng_ip_pool*)pools, n_pools, (const bng_server_config*)cfg,
      (unsigned long long*)stats, now_sec, (const uint64_t*)now_ptr);
}

void bng_launch_dhcp_service(void* ctrl, void* req, const void* in_len,
                             void* out_len, void* verdict, void* scratch,
                             int n_slots, int n_blocks, void* ctrs,
                             const void* subs,
                             uint32_t sub_mask, const void* pools,
                             uint32_t n_pools, const void* cfg, void* stats,
                             hipStream_t s) {
  hipLaunchKernelGGL(dhcp_service_kernel, dim3(n_blocks), dim3(256), 0, s,
      (bng_svc_ctrl*)ctrl, (uint8_t*)req, (const uint16_t*)in_len,
      (uint16_t*)out_len, (uint8_t*)verdict, (uint8_t*)scratch, n_slots,
      (uint32_t*)ctrs,
      (const bng_sub_entry*)subs, sub_mask, (const bng_ip_pool*)pools,
      n_pools, (const bng_server_config*)cfg,
      (unsigned long long*)stats);
}

void bng_launch_nat44(void* data, const void* in_len, void* verdict, int n,
                      int stride, int is_egress,
                      void* sessions, uint32_t sess_mask,
                      void* reverse, uint32_t rev_mask,
                      void* eim, uint32_t eim_mask,
                      void* subnat, uint32_t subnat_mask,
                      const void* cfg, const void* hairpin,
                      uint32_t n_hairpin, void* stats,
                      void* log_ring, void* log_hdr, uint64_t now_ns,
                      hipStream_t s) {
  hipLaunchKernelGGL(nat44_kernel, dim3(pkt_grid(n)), dim3(256), 0, s,
      (uint8_t*)data, (const uint16_t*)in_len, (uint8_t*)verdict, n, stride,
      is_egress, (bng_nat_session*)sessions, sess_mask,
      (bng_nat_reverse*)reverse, rev_mask, (bng_eim_entry*)eim, eim_mask,
      (bng_subctx*)subnat, subnat_mask, (const bng_nat_config*)cfg,
      (const uint32_t*)hairpin, n_hairpin, (unsigned long long*)stats,
      (bng_nat_log_entry*)log_ring, (bng_ring_header*)log_hdr, now_ns);
}

void bng_launch_qos(void* data, const void* in_len, void* verdict, int n,
                    int stride, int is_egress, void* table, uint32_t mask,
                    void* stats, uint64_t now_ns, hipStream_t s) {
  hipLaunchKernelGGL(qos_kernel, dim3(pkt_grid(n)), dim3(256), 0, s,
      (uint8_t*)data, (const uint16_t*)in_len, (uint8_t*)verdict, n, stride,
      is_egress, table, mask, (unsigned long long*)stats,
      now_ns);
}

void bng_launch_antispoof(void* data, const void* in_len, void* verdict,
                          int n, int stride, const void* bindings,
                          uint32_t bmask, const void* cfg, void* stats,
                          void* ring, void* hdr, uint64_t now_ns,
                          hipStream_t s) {
  hipLaunchKernelGGL(antispoof_kernel, dim3(pkt_grid(n)), dim3(256), 0, s,
      (uint8_t*)data, (const uint16_t*)in_len, (uint8_t*)verdict, n, stride,
      (const bng_binding_entry*)bindings, bmask,
      (const bng_antispoof_config*)cfg, (unsigned long long*)stats,
      (bng_spoof_event*)ring, (bng_ring_header*)hdr, now_ns);
}

void bng_launch_uplink(bng_uplink_params* P, hipStream_t s) {
  hipLaunchKernelGGL(uplink_pipeline_kernel, dim3(pkt_grid(P->n)), dim3(256),
                     0, s, *P);
}

void bng_launch_downlink(bng_uplink_params* P, hipStream_t s) {
  hipLaunchKernelGGL(downlink_pipeline_kernel, dim3(pkt_grid(P->n)),
                     dim3(256), 0, s, *P);
}

void bng_launch_pkt_class(const void* data, const void* in_len, void* cls,
                          int n, int stride, hipStream_t s) {
  hipLaunchKernelGGL(pkt_class_kernel, dim3(aux_grid(n)), dim3(256), 0, s,
      (const uint8_t*)data, (const uint16_t*)in_len, (uint8_t*)cls, n,
      stride);
}

void bng_launch_sub_upsert(void* t, uint32_t mask, const void* batch, int n,
                           void* rc, hipStream_t s) {
  hipLaunchKernelGGL(sub_upsert_kernel, dim3((n + 255) / 256), dim3(256), 0,
      s, (bng_sub_entry*)t, mask, (const bng_sub_entry*)batch, n, (int*)rc);
}
void bng_launch_sess_import(void* sess, uint32_t sess_mask, void* rev,
                            uint32_t rev_mask, void* eim, uint32_t eim_mask,
                            const void* batch, int n, void* rc,
                            hipStream_t s) {
  hipLaunchKernelGGL(sess_import_kernel, dim3((n + 255) / 256), dim3(256),
      0, s, (bng_nat_session*)sess, sess_mask, (bng_nat_reverse*)rev,
      rev_mask, (bng_eim_entry*)eim, eim_mask,
      (const bng_sess_export*)batch, n, (int*)rc);
}
void bng_launch_sub_delete(void* t, uint32_t mask, const void* keys, int n,
                           hipStream_t s) {
  hipLaunchKernelGGL(sub_delete_kernel, dim3((n + 255) / 256), dim3(256), 0,
      s, (bng_sub_entry*)t, mask, (const uint64_t*)keys, n);
}
void bng_launch_subctx_upsert(void* t, uint32_t mask, const void* batch,
                              int n, uint32_t um, void* rc, hipStream_t s) {
  hipLaunchKernelGGL(subctx_upsert_kernel, dim3((n + 255) / 256), dim3(256),
      0, s, (bng_subctx*)t, mask, (const bng_subctx*)batch, n, um,
      (int*)rc);
}
void bng_launch_qos_upsert(void* t, uint32_t mask, const void* batch, int n,
                           void* rc, hipStream_t s) {
  hipLaunchKernelGGL(qos_upsert_kernel, dim3((n + 255) / 256), dim3(256), 0,
      s, (bng_qos_bucket*)t, mask, (const bng_qos_bucket*)batch, n, (int*)rc);
}
void bng_launch_binding_upsert(void* t, uint32_t mask, const void* batch,
                               int n, void* rc, hipStream_t s) {
  hipLaunchKernelGGL(binding_upsert_kernel, dim3((n + 255) / 256), dim3(256),
      0, s, (bng_binding_entry*)t, mask, (const bng_binding_entry*)batch, n,
      (int*)rc);
}
void bng_launch_binding_delete(void* t, uint32_t mask, const void* keys,
                               int n, hipStream_t s) {
  hipLaunchKernelGGL(binding_delete_kernel, dim3((n + 255) / 256), dim3(256),
      0, s, (bng_binding_entry*)t, mask, (const uint64_t*)keys, n);
}

void bng_launch_nat_sweep(void* sessions, uint32_t n_slots, void* reverse,
                          uint32_t rev_mask, void* subnat,
                          uint32_t subnat_mask, void* eim,
                          uint32_t eim_slots, uint64_t eim_to,
                          uint64_t now_ns,
                          uint64_t udp_to, uint64_t tcp_est_to,
                          uint64_t tcp_tr_to, uint64_t icmp_to, void* stats,
                          hipStream_t s) {
  hipLaunchKernelGGL(nat_sweep_kernel, dim3(2048), dim3(256), 0, s,
      (bng_nat_session*)sessions, n_slots, (bng_nat_reverse*)reverse,
      rev_mask, (bng_subctx*)subnat, subnat_mask, (bng_eim_entry*)eim,
      eim_slots, eim_to, now_ns, udp_to,
      tcp_est_to, tcp_tr_to, icmp_to, (unsigned long long*)stats);
}

void bng_launch_pppoe_decap(void* data, void* in_len, void* state, int n,
                            int stride, const void* sess, void* stats,
                            hipStream_t s) {
  hipLaunchKernelGGL(pppoe_decap_kernel, dim3(pkt_grid(n)), dim3(256), 0, s,
      (uint8_t*)data, (uint16_t*)in_len, (uint8_t*)state, n, stride,
      (const bng_pppoe_sess*)sess, (unsigned long long*)stats);
}

void bng_launch_pppoe_encap(void* data, void* in_len, void* verdict,
                            void* state, int n, int stride,
                            const void* by_ip, uint32_t ip_mask,
                            const void* sess, const void* scfg, void* stats,
                            hipStream_t s) {
  hipLaunchKernelGGL(pppoe_encap_kernel, dim3(pkt_grid(n)), dim3(256), 0, s,
      (uint8_t*)data, (uint16_t*)in_len, (uint8_t*)verdict, (uint8_t*)state,
      n, stride, (const bng_pppoe_ip*)by_ip, ip_mask,
      (const bng_pppoe_sess*)sess, (const bng_server_config*)scfg,
      (unsigned long long*)stats);
}

void bng_launch_pppoe_sess_upsert(void* sess, void* by_ip, uint32_t ip_mask,
                                  const void* batch, int n, void* rc,
                                  hipStream_t s) {
  hipLaunchKernelGGL(pppoe_sess_upsert_kernel, dim3((n + 255) / 256),
      dim3(256), 0, s, (bng_pppoe_sess*)sess, (bng_pppoe_ip*)by_ip, ip_mask,
      (const bng_pppoe_sess*)batch, n, (int*)rc);
}

void bng_launch_pppoe_sess_delete(void* sess, void* by_ip, uint32_t ip_mask,
                                  const void* sids, int n, hipStream_t s) {
  hipLaunchKernelGGL(pppoe_sess_delete_kernel, dim3((n + 255) / 256),
      dim3(256), 0, s, (bng_pppoe_sess*)sess, (bng_pppoe_ip*)by_ip, ip_mask,
      (const int32_t*)sids, n);
}

void bng_set_acct_combine(int rounds) { g_acct_rounds = rounds; }
int bng_get_acct_combine(void) { return g_acct_rounds; }

void bng_launch_acct_resolve(const void* data, const void* in_len,
                             void* slot, int n, int stride,
                             const void* table, uint32_t mask,
                             hipStream_t s) {
  hipLaunchKernelGGL(acct_resolve_kernel, dim3(pkt_grid(n)), dim3(256), 0, s,
      (const uint8_t*)data, (const uint16_t*)in_len, (int32_t*)slot, n,
      stride, (const bng_acct_entry*)table, mask);
}

void bng_launch_acct_commit(void* table, uint32_t mask, const void* slot,
                            const void* verdict, const void* out_len, int n,
                            uint64_t now_ns, hipStream_t s) {
  hipLaunchKernelGGL(acct_commit_kernel, dim3(pkt_grid(n)), dim3(256), 0, s,
      (bng_acct_entry*)table, mask, (const int32_t*)slot,
      (const uint8_t*)verdict, (const uint16_t*)out_len, n, now_ns,
      g_acct_rounds);
}

void bng_launch_acct_downlink(const void* data, const void* in_len,
                              const void* verdict, int n, int stride,
                              void* table, uint32_t mask, uint64_t now_ns,
                              hipStream_t s) {
  hipLaunchKernelGGL(acct_downlink_kernel, dim3(pkt_grid(n)), dim3(256), 0,
      s, (const uint8_t*)data, (const uint16_t*)in_len,
      (const uint8_t*)verdict, n, stride, (bng_acct_entry*)table, mask,
      now_ns, g_acct_rounds);
}

void bng_launch_acct_upsert(void* table, uint32_t mask, const void* ips,
                            int n, int reset, void* rc, hipStream_t s) {
  hipLaunchKernelGGL(acct_upsert_kernel, dim3((n + 255) / 256), dim3(256), 0,
      s, (bng_acct_entry*)table, mask, (const uint32_t*)ips, n, reset,
      (int*)rc);
}

void bng_launch_acct_read(void* table, uint32_t mask, const void* ips, int n,
                          void* out, hipStream_t s) {
  hipLaunchKernelGGL(acct_read_kernel, dim3((n + 255) / 256), dim3(256), 0,
      s, (bng_acct_entry*)table, mask, (const uint32_t*)ips, n,
      (bng_acct_entry*)out);
}

void bng_launch_acct_delete(void* table, uint32_t mask, const void* ips,
                            int n, void* out, hipStream_t s) {
  hipLaunchKernelGGL(acct_delete_kernel, dim3((n + 255) / 256), dim3(256), 0,
      s, (bng_acct_entry*)table, mask, (const uint32_t*)ips, n,
      (bng_acct_entry*)out);
}

void bng_launch_wg_uplink(const void* data, const void* in_len,
                          void* verdict, void* out_len, void* gate,
                          const void* order_in, void* order_out, int n,
                          int stride, const void* table, uint32_t mask,
                          const void* cfg, void* stats, hipStream_t s) {
  hipLaunchKernelGGL(wg_uplink_kernel, dim3(pkt_grid(n)), dim3(256), 0, s,
      (const uint8_t*)data, (const uint16_t*)in_len, (uint8_t*)verdict,
      (uint16_t*)out_len, (uint8_t*)gate, (const int32_t*)order_in,
      (int32_t*)order_out, n, stride, (const bng_wg_entry*)table, mask,
      (const bng_wg_config*)cfg, (unsigned long long*)stats);
}

void bng_launch_wg_downlink(const void* data, const void* in_len,
                            void* verdict, void* gate, int n, int stride,
                            const void* table, uint32_t mask,
                            const void* cfg, void* stats, hipStream_t s) {
  hipLaunchKernelGGL(wg_downlink_kernel, dim3(pkt_grid(n)), dim3(256), 0, s,
      (const uint8_t*)data, (const uint16_t*)in_len, (uint8_t*)verdict,
      (uint8_t*)gate, n, stride, (const bng_wg_entry*)table, mask,
      (const bng_wg_config*)cfg, (unsigned long long*)stats);
}

void bng_launch_wg_upsert(void* table, uint32_t mask, const void* batch,
                          int n, void* rc, hipStream_t s) {
  hipLaunchKernelGGL(wg_upsert_kernel, dim3((n + 255) / 256), dim3(256), 0,
      s, (bng_wg_entry*)table, mask, (const bng_wg_entry*)batch, n,
      (int*)rc);
}

void bng_launch_wg_delete(void* table, uint32_t mask, const void* ips, int n,
                          hipStream_t s) {
  hipLaunchKernelGGL(wg_delete_kernel, dim3((n + 255) / 256), dim3(256), 0,
      s, (bng_wg_entry*)table, mask, (const uint32_t*)ips, n);
}

void bng_launch_shard_owner(const void* data, const void* in_len,
                            void* owner, int n, int stride, int n_shards,
                            hipStream_t s) {
  hipLaunchKernelGGL(shard_owner_kernel, dim3(aux_grid(n)), dim3(256), 0, s,
      (const uint8_t*)data, (const uint16_t*)in_len, (int32_t*)owner, n,
      stride, n_shards);
}

} /* extern "C" */
