/* bng_abi.h — the host<->device table ABI for the MI355X BNG dataplane.
 *
 * This is the MI355X-native analog of the reference's eBPF map contract
 * (reference: bpf/maps.h:89-234, bpf/nat44.c:92-320, bpf/qos_ratelimit.c:24-65,
 * bpf/antispoof.c:36-119).  Every table lives in HBM3E as a fixed-capacity
 * open-addressing hash table (power-of-2 slots, linear probing) or a flat
 * array.  The Python side mirrors these structs byte-for-byte in
 * bng_amd/dataplane/abi.py; tests/test_abi.py asserts the layouts agree
 * (the analog of the reference's test/ebpf/maps_test.go struct-ABI tests).
 *
 * Design departures from the reference (deliberate, GPU-first):
 *  - One unified subscriber table replaces the reference's three maps
 *    (subscriber_pools / vlan_subscriber_pools / circuit_id_subscribers,
 *    bpf/maps.h:99-129,229-234): the 64-bit key space is tagged by source
 *    (MAC / QinQ VLAN / circuit-ID FNV hash) so the fast path probes ONE
 *    HBM table at most three times instead of three tables.
 *  - BPF LRU maps become timeout-reclaimed open-addressing tables: a probe
 *    that hits an expired entry may reclaim the slot with atomicCAS.
 *  - bpf_ktime_get_ns() per packet becomes one host-written batch timestamp.
 *  - Per-CPU stats maps become one device-global atomic counter block
 *    (256 CUs' contention on ~10 u64 counters is negligible per batch).
 */
#ifndef BNG_ABI_H
#define BNG_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- sizing */
enum {
  BNG_MAX_SUBSCRIBERS_LOG2 = 21, /* 2M slots for 1M subscribers (load<=0.5) */
  BNG_MAX_POOLS            = 16384,
  BNG_MAX_NAT_SESSIONS_LOG2= 23, /* 8M slots for 4M sessions */
  BNG_MAX_EIM_LOG2         = 22, /* 4M slots for 2M EIM mappings */
  BNG_MAX_SUBNAT_LOG2      = 21,
  BNG_MAX_QOS_LOG2         = 21,
  BNG_MAX_BINDINGS_LOG2    = 21,
  BNG_MAX_ACCT_LOG2        = 21, /* 2M slots for 1M accounted subscribers  */
  BNG_MAX_WG_LOG2          = 21, /* 2M slots for 1M quarantined subscribers */
  BNG_MAX_WG_ALLOWED       = 64, /* walled-garden (ip, port, proto) keys    */
  BNG_MAX_WG_REDIRECT_PORTS = 8,
  BNG_MAX_PROBE            = 128, /* linear-probe bound before declaring full */
  BNG_MAX_PRIVATE_RANGES   = 64,  /* bpf/nat44.c:314-320 nat_private_ranges */
  BNG_MAX_ALLOWED_RANGES   = 256, /* bpf/antispoof.c:113-119 allowed_ranges_v4 */
  BNG_MAX_HAIRPIN_IPS      = 1024,
  BNG_MAX_ALG_PORTS        = 64,
  BNG_LOG_RING_LOG2        = 15,  /* 32k nat-log entries (~1.25MB; ref 1MB rb) */
  BNG_SPOOF_RING_LOG2      = 14,
};

/* key-space tags for the unified subscriber table (bits 63:62 of the key) */
#define BNG_KEY_MAC      0ULL   /* key = MAC as u64 (< 2^48)               */
#define BNG_KEY_VLAN     (1ULL << 62)  /* key = tag | s_tag<<16 | c_tag    */
#define BNG_KEY_CIRCUIT  (2ULL << 62)  /* key = tag | (fnv1a64(cid) >> 2)  */
#define BNG_KEY_EMPTY    0ULL
#define BNG_KEY_TOMBSTONE 0xFFFFFFFFFFFFFFFFULL

/* ----------------------------------------------------- verdicts (XDP/TC) */
enum bng_verdict {
  BNG_PASS = 0,  /* to slow path (XDP_PASS / TC_ACT_OK untouched)          */
  BNG_TX   = 1,  /* reply built in place, transmit (XDP_TX)                */
  BNG_DROP = 2,  /* drop (XDP_DROP / TC_ACT_SHOT)                          */
  BNG_FWD  = 3,  /* packet rewritten, forward (TC_ACT_OK after NAT)        */
};

/* ------------------------------------------------- subscriber fast path */
/* Unified subscriber entry: reference pool_assignment (bpf/maps.h:89-97)
 * plus its hash key; 32 bytes = half a cache line, 2 entries per 64B line. */
typedef struct bng_sub_entry {
  uint64_t key;          /* tagged key; 0 empty, ~0 tombstone              */
  uint32_t pool_id;
  uint32_t allocated_ip; /* network byte order, as it appears in packets   */
  uint64_t lease_expiry; /* unix seconds (ref maps.h:94)                   */
  uint16_t vlan_id;
  uint8_t  client_class;
  uint8_t  flags;
  uint32_t _pad;
} bng_sub_entry;  /* 32 B */

/* IP pool metadata, flat array indexed by pool_id (ref maps.h:135-151). */
typedef struct bng_ip_pool {
  uint32_t network;      /* network byte order */
  uint32_t gateway;
  uint32_t dns_primary;
  uint32_t dns_secondary;
  uint32_t lease_time;   /* host order, seconds */
  uint8_t  prefix_len;
  uint8_t  valid;
  uint16_t _pad;
  uint32_t _pad2;
} bng_ip_pool;  /* 28 B -> padded */

typedef struct bng_server_config {   /* ref maps.h:154-159 */
  uint8_t  server_mac[6];
  uint16_t _pad;
  uint32_t server_ip;    /* network byte order */
  uint32_t if_index;
} bng_server_config;  /* 16 B */

/* DHCP fast-path counters, same order as ref maps.h:171-184. */
enum bng_dhcp_stat {
  BNG_ST_TOTAL_REQUESTS = 0,
  BNG_ST_FASTPATH_HITS,
  BNG_ST_FASTPATH_MISSES,
  BNG_ST_ERRORS,
  BNG_ST_CACHE_EXPIRED,
  BNG_ST_OPTION82_PRESENT,
  BNG_ST_OPTION82_ABSENT,
  BNG_ST_BROADCAST_REPLIES,
  BNG_ST_UNICAST_REPLIES,
  BNG_ST_VLAN_PACKETS,
  BNG_DHCP_NSTATS
};

/* --------------------------------------------------------------- NAT44 */
/* 5-tuple (ref nat44.c:92-99). 16 B, hashed into a 64-bit slot signature. */
typedef struct bng_nat_tuple {
  uint32_t src_ip;   /* network order */
  uint32_t dst_ip;
  uint16_t src_port; /* network order */
  uint16_t dst_port;
  uint8_t  protocol;
  uint8_t  _pad[3];
} bng_nat_tuple;  /* 16 B */

enum bng_nat_state {   /* ref nat44.c:65-71 */
  BNG_NAT_NEW = 0, BNG_NAT_ESTABLISHED = 1, BNG_NAT_FIN_WAIT = 2,
  BNG_NAT_CLOSING = 3, BNG_NAT_TIME_WAIT = 4,
};

/* Session entry: 128 B = 2 cache lines; line 0 is the hot lookup+translate
 * path, line 1 the accounting (ref nat_session nat44.c:123-141). */
typedef struct bng_nat_session {
  uint64_t sig;          /* 0 empty, ~0 tombstone, else mix64(tuple)|1     */
  bng_nat_tuple key;     /* full key for verification after sig match      */
  uint32_t nat_ip;
  uint16_t nat_port;     /* network order */
  uint16_t orig_port;    /* network order */
  uint32_t orig_ip;
  uint8_t  state;
  uint8_t  is_hairpin;
  uint8_t  ready;        /* set (agent-scope release) after fields written */
  uint8_t  _pad;
  uint64_t last_seen;    /* ns */
  /* ---- line 1 ---- */
  uint64_t created;
  uint64_t packets_out;
  uint64_t packets_in;
  uint64_t bytes_out;
  uint64_t bytes_in;
  uint64_t _pad2[5];
} bng_nat_session;  /* 128 B */

/* Reverse map entry: external tuple -> internal tuple (ref nat44.c:228-233) */
typedef struct bng_nat_reverse {
  uint64_t sig;
  bng_nat_tuple key;     /* external-side tuple */
  bng_nat_tuple orig;    /* original internal tuple */
  uint8_t  ready;
  uint8_t  _pad[7];
} bng_nat_reverse;  /* 48 B */

/* EIM entry (RFC 4787; ref eim_key/eim_mapping nat44.c:104-120). */
typedef struct bng_eim_entry {
  uint64_t sig;          /* mix of (internal_ip, internal_port, proto)     */
  uint32_t internal_ip;
  uint16_t internal_port; /* network order */
  uint8_t  protocol;
  uint8_t  ready;
  uint32_t external_ip;
  uint16_t external_port; /* HOST order, as in ref eim_mapping             */
  uint16_t _pad;
  uint64_t created;
  uint64_t last_used;
  uint32_t ref_count;
  uint32_t flags;
} bng_eim_entry;  /* 48 B */

/* Per-subscriber port block + counters (ref port_block/subscriber_nat
 * nat44.c:144-164).  Host-inserted (stream-ordered), device-updated. */
/* Per-subscriber UPLINK CONTEXT — the RFC6431 port block (ref
 * subscriber_nat nat44.c:157-164) and the ingress token bucket (ref
 * qos_ingress qos_ratelimit.c:44-50) merged into ONE 64-byte entry
 * keyed by the subscriber IP: the fused uplink pipeline pays a single
 * random HBM touch for both stages (measured: each separate table walk
 * costs ~0.2-0.4 ns/packet, profiles/kernel_stats_r01.md). */
typedef struct bng_subctx {
  uint32_t key_ip;       /* subscriber private IP; 0 = empty            */
  uint32_t public_ip;    /* NAT public IP; nat_valid gates              */
  uint16_t port_start;   /* host order, inclusive                       */
  uint16_t port_end;
  uint8_t  qos_valid;    /* upload policy installed                     */
  uint8_t  nat_valid;    /* port block installed                        */
  uint8_t  priority;
  uint8_t  flags;
  uint64_t rate_bps;     /* 0 = unlimited                               */
  int64_t  tokens;       /* device atomics                              */
  uint64_t last_update;  /* ns; refill-claim CAS                        */
  uint32_t burst_bytes;
  uint32_t next_port;    /* atomic rotor (session-create path only)     */
  uint32_t subscriber_id;
  uint32_t sessions_active;   /* device atomics                         */
  uint32_t sessions_total;
  uint32_t _pad;
} bng_subctx;  /* 64 B; bytes 0-23 carry everything the per-packet hot
                  path needs (key, NAT identity, validity, rate) */

/* subctx upsert merge masks */
#define BNG_CTX_SET_NAT 1u
#define BNG_CTX_SET_QOS 2u
#define BNG_CTX_CLR_QOS 4u
#define BNG_CTX_CLR_NAT 8u

/* Global NAT config (ref nat_config nat44.c:271-277). */
#define BNG_NAT_FLAG_EIM       0x01
#define BNG_NAT_FLAG_EIF       0x02
#define BNG_NAT_FLAG_HAIRPIN   0x04
#define BNG_NAT_FLAG_ALG_FTP   0x08
#define BNG_NAT_FLAG_ALG_SIP   0x10
#define BNG_NAT_FLAG_PARITY    0x20
#define BNG_NAT_FLAG_CONTIG    0x40
#define BNG_NAT_FLAG_ICMP_ERR  0x80  /* translate inbound ICMP errors (RFC 5508) */

typedef struct bng_nat_config {
  uint32_t flags;
  uint16_t port_range_start;
  uint16_t port_range_end;
  uint32_t default_ports_per_sub;
  uint32_t n_private_ranges;
  uint32_t n_alg_ports;
  uint32_t _pad;
  /* private ranges as SORTED, MERGED host-order intervals [lo, hi];
   * the ref uses an LPM trie for a membership test (nat44.c:314-320) —
   * the GPU equivalent is a binary search over an L2-resident interval
   * table (the launcher folds {net, mask} prefixes into intervals; the
   * cap matches the ref trie's max_entries sizing). */
  uint32_t priv_lo[BNG_MAX_PRIVATE_RANGES];
  uint32_t priv_hi[BNG_MAX_PRIVATE_RANGES];
  uint32_t alg_key[BNG_MAX_ALG_PORTS];   /* port<<16 | proto (host order)  */
} bng_nat_config;

enum bng_nat_stat {  /* ref nat_stats nat44.c:176-190 */
  BNG_NS_SNAT = 0, BNG_NS_DNAT, BNG_NS_HAIRPIN, BNG_NS_DROPPED, BNG_NS_PASSED,
  BNG_NS_SESS_CREATED, BNG_NS_SESS_EXPIRED, BNG_NS_PORT_EXHAUSTION,
  BNG_NS_EIM_HITS, BNG_NS_EIM_MISSES, BNG_NS_ALG_TRIGGERS,
  BNG_NS_CT_LOOKUPS, BNG_NS_CT_HITS,
  /* no reference analog: inbound ICMP errors under BNG_NAT_FLAG_ICMP_ERR */
  BNG_NS_ICMP_ERR_XLATE, BNG_NS_ICMP_ERR_NOMAP,
  BNG_NAT_NSTATS
};

/* NAT compliance log record (ref nat_log_entry nat44.c:193-205); ring. */
enum bng_nat_log_event {  /* ref nat44.c:74-82 */
  BNG_LOG_SESSION_CREATE = 1, BNG_LOG_SESSION_DELETE = 2,
  BNG_LOG_PB_ASSIGN = 3, BNG_LOG_PB_RELEASE = 4, BNG_LOG_PORT_EXHAUSTION = 5,
  BNG_LOG_HAIRPIN = 6, BNG_LOG_ALG_TRIGGER = 7,
};

typedef struct bng_nat_log_entry {
  uint64_t timestamp;
  uint32_t event_type;
  uint32_t subscriber_id;
  uint32_t private_ip;
  uint32_t public_ip;
  uint16_t private_port;
  uint16_t public_port;
  uint32_t dest_ip;
  uint16_t dest_port;
  uint8_t  protocol;
  uint8_t  flags;
} bng_nat_log_entry;  /* 40 B */

/* ------------------------------------------------------------------ QoS */
/* Token bucket (ref token_bucket qos_ratelimit.c:24-31).  tokens is a
 * SIGNED 64-bit so consume can be one atomicAdd(-len) with undo-on-negative
 * (the reference's per-packet read-modify-write is a data race it tolerates;
 * ours is an atomic with a bounded transient-negative race). */
typedef struct bng_qos_bucket {
  uint32_t key_ip;       /* subscriber IP (network order); 0 empty         */
  uint8_t  valid;
  uint8_t  priority;
  uint16_t _pad;
  uint64_t rate_bps;     /* 0 = unlimited */
  int64_t  tokens;       /* bytes */
  uint64_t last_update;  /* ns */
  uint32_t burst_bytes;
  uint32_t _pad2;
  uint64_t _pad3[3];
} bng_qos_bucket;  /* 64 B */

enum bng_qos_stat {  /* ref qos_stats qos_ratelimit.c:53-58 */
  BNG_QS_PKT_PASSED = 0, BNG_QS_PKT_DROPPED, BNG_QS_BYTES_PASSED,
  BNG_QS_BYTES_DROPPED, BNG_QOS_NSTATS
};

/* ------------------------------------------------------------ antispoof */
enum bng_antispoof_mode {  /* ref antispoof.c:30-33 */
  BNG_AS_DISABLED = 0, BNG_AS_STRICT = 1, BNG_AS_LOOSE = 2, BNG_AS_LOG_ONLY = 3,
};

typedef struct bng_binding_entry {  /* ref subscriber_binding antispoof.c:36-43 */
  uint64_t key_mac;      /* MAC as u64; 0 empty, ~0 tombstone              */
  uint32_t ipv4_addr;    /* network order */
  uint8_t  ipv4_valid;
  uint8_t  ipv6_valid;
  uint8_t  mode;
  uint8_t  _pad;
  uint8_t  ipv6_addr[16];
} bng_binding_entry;  /* 32 B */

typedef struct bng_antispoof_config {  /* ref antispoof.c:79-83 */
  uint8_t  default_mode;
  uint8_t  log_violations;
  uint16_t _pad;
  uint32_t n_allowed_ranges;
  /* sorted merged host-order intervals, like bng_nat_config (ref
   * allowed_ranges_v4 LPM trie, antispoof.c:113-119) */
  uint32_t allowed_lo[BNG_MAX_ALLOWED_RANGES];
  uint32_t allowed_hi[BNG_MAX_ALLOWED_RANGES];
} bng_antispoof_config;

enum bng_antispoof_stat {  /* ref antispoof_stats antispoof.c:58-65 */
  BNG_AS_ALLOWED = 0, BNG_AS_DROPPED, BNG_AS_LOGGED,
  BNG_AS_V4_VIOLATIONS, BNG_AS_V6_VIOLATIONS, BNG_AS_UNKNOWN_MAC,
  BNG_AS_NSTATS
};

typedef struct bng_spoof_event {  /* ref spoof_event antispoof.c:46-55 */
  uint64_t timestamp;
  uint8_t  src_mac[6];
  uint8_t  protocol;   /* 4 or 6 */
  uint8_t  _pad;
  uint32_t spoofed_ip;
  uint32_t allowed_ip;
  uint8_t  spoofed_ipv6[16];
  uint8_t  allowed_ipv6[16];
} bng_spoof_event;  /* 56 B */

/* ---------------------------------------------- PPPoE session-data path */
/* Per-session entry of the PPPoE fast path, a flat array direct-indexed
 * by the 16-bit PPPoE session id (65536 entries, 1 MiB: no hash, no
 * probe).  One 16-B load serves a packet.  No reference analog — the
 * reference terminates PPPoE entirely in user space. */
#define BNG_PPPOE_MAX_SESSIONS 65536
#define BNG_PPPOE_MAC_MASK     0x0000FFFFFFFFFFFFULL
#define BNG_PPPOE_VALID        (1ULL << 63)

typedef struct bng_pppoe_sess {
  uint64_t mac_valid;   /* bits 47:0 client MAC (as mac_to_u64), bit 63 valid */
  uint32_t ip;          /* subscriber IPv4, host int of the BE field        */
  uint16_t mru;         /* peer MRU: largest IP packet the client accepts   */
  uint16_t session_id;  /* == the entry's index; the upsert batch's key     */
} bng_pppoe_sess;  /* 16 B */

/* Subscriber IP -> session, for the downlink encap: open-addressing table
 * with the usual EMPTY / TOMBSTONE keys and BNG_MAX_PROBE bound. */
#define BNG_PPPOE_IP_KEY(ip) ((1ULL << 32) | (uint64_t)(uint32_t)(ip))

typedef struct bng_pppoe_ip {
  uint64_t key;         /* BNG_PPPOE_IP_KEY(ip); 0 empty, ~0 tombstone      */
  uint64_t sid_mac;     /* bits 63:48 session id, bits 47:0 client MAC      */
} bng_pppoe_ip;  /* 16 B */

enum bng_pppoe_stat {
  BNG_PS_DECAP_OK = 0, BNG_PS_DECAP_CTRL, BNG_PS_DECAP_UNKNOWN_SESSION,
  BNG_PS_DECAP_MAC_MISMATCH, BNG_PS_DECAP_MALFORMED,
  BNG_PS_ENCAP_OK, BNG_PS_ENCAP_TOO_BIG, BNG_PS_ENCAP_NO_ROOM,
  BNG_PPPOE_NSTATS
};

/* per-packet state written by the decap / encap kernels */
enum bng_pppoe_state {
  BNG_PPPOE_NONE = 0,    /* not a PPPoE session frame / no session: untouched */
  BNG_PPPOE_DECAP = 1,   /* uplink: header removed, now an IPoE frame         */
  BNG_PPPOE_CTRL = 2,    /* uplink: PPP control protocol, for the host server */
  BNG_PPPOE_REJECT = 3,  /* uplink: malformed / unknown session / wrong MAC   */
  BNG_PPPOE_ENCAP = 4,   /* downlink: header added                            */
  BNG_PPPOE_TOO_BIG = 5, /* downlink: exceeds the peer MRU, verdict -> PASS   */
  BNG_PPPOE_NO_ROOM = 6, /* downlink: row too short for +8 B, verdict -> PASS */
};

/* ------------------------------------------- per-subscriber accounting */
/* Traffic counters of one subscriber, the source of the RADIUS
 * Acct-Input/Output-Octets/Packets (ref pkg/radius/client.go:289-304).
 * One cache line per entry, keyed by the subscriber IPv4 (the integer
 * ip2u32 yields and add_subscriber_nat takes).  Open addressing with the
 * usual EMPTY / TOMBSTONE keys and BNG_MAX_PROBE bound.  Host-inserted
 * (stream-ordered), device-updated with relaxed agent-scope atomics. */
#define BNG_ACCT_KEY(ip) ((1ULL << 32) | (uint64_t)(uint32_t)(ip))  /* never 0 / ~0 */

typedef struct bng_acct_entry {
  uint64_t key;            /* BNG_ACCT_KEY(ip); 0 empty, ~0 tombstone          */
  uint64_t up_bytes;       /* forwarded subscriber -> core                      */
  uint64_t up_pkts;
  uint64_t down_bytes;     /* forwarded core -> subscriber                      */
  uint64_t down_pkts;
  uint64_t up_drop_pkts;   /* verdict DROP (antispoof / NAT / QoS), uplink      */
  uint64_t down_drop_pkts;
  uint64_t last_seen;      /* batch now_ns of the last FORWARDED packet         */
} bng_acct_entry;  /* 64 B */

/* ------------------------------------------------- walled-garden gate */
/* Quarantine state of one subscriber address, consulted for every untagged
 * IPv4 data frame in both directions by the gate kernels around the fused
 * pipelines.  No reference analog: the reference keeps the walled-garden
 * state machine in user space (pkg/walledgarden/manager.go) and has no
 * walled_garden.c.  Keyed by the subscriber IPv4 like the accounting table;
 * one 16-B load serves a probe step.  Open addressing with the usual
 * EMPTY / TOMBSTONE keys and BNG_MAX_PROBE bound; host-inserted
 * (stream-ordered), read-only for the packet kernels. */
#define BNG_WG_KEY(ip) ((1ULL << 32) | (uint64_t)(uint32_t)(ip))  /* never 0 / ~0 */
#define BNG_WG_MAC_MASK    0x0000FFFFFFFFFFFFULL
#define BNG_WG_STATE_SHIFT 56

enum bng_wg_state {
  BNG_WG_WALLED  = 1,  /* quarantined: allow-list, portal redirect, else drop */
  BNG_WG_BLOCKED = 2,  /* no service at all                                  */
};

typedef struct bng_wg_entry {
  uint64_t key;        /* BNG_WG_KEY(ip); 0 empty, ~0 tombstone             */
  uint64_t mac_state;  /* bits 47:0 subscriber MAC (as mac_to_u64),
                          bits 63:56 bng_wg_state                           */
} bng_wg_entry;  /* 16 B */

/* What a quarantined subscriber may reach.  allowed_key is sorted and
 * unique, allowed_ip holds the sorted distinct addresses of those keys
 * (the any-port rule for frames without readable ports); both are
 * binary-searched. */
typedef struct bng_wg_config {
  uint32_t n_allowed;
  uint32_t n_allowed_ips;
  uint32_t n_redirect_ports;
  uint32_t _pad;
  uint64_t allowed_key[BNG_MAX_WG_ALLOWED];  /* ip<<32 | port<<16 | proto,
                                                host order                  */
  uint32_t allowed_ip[BNG_MAX_WG_ALLOWED];
  uint16_t redirect_port[BNG_MAX_WG_REDIRECT_PORTS];  /* TCP, to the host   */
} bng_wg_config;  /* 800 B */

/* per-packet gate code written by the gate kernels */
enum bng_wg_gate {
  BNG_WG_NONE = 0,      /* not in the garden: the pipeline's verdict stands */
  BNG_WG_ALLOW,         /* allow-listed: FWD, bytes untouched, no NAT       */
  BNG_WG_REDIRECT,      /* uplink HTTP: PASS, the host redirects            */
  BNG_WG_DROP_WALLED,
  BNG_WG_DROP_BLOCKED,
  BNG_WG_DROP_MAC,      /* uplink: source MAC is not the quarantined one    */
};

enum bng_wg_stat {
  BNG_WS_UP_ALLOWED = 0, BNG_WS_UP_REDIRECTED, BNG_WS_UP_DROP_WALLED,
  BNG_WS_UP_DROP_BLOCKED, BNG_WS_UP_DROP_MAC,
  BNG_WS_DOWN_ALLOWED, BNG_WS_DOWN_DROP_WALLED, BNG_WS_DOWN_DROP_BLOCKED,
  BNG_WG_NSTATS
};

/* ----------------------------------------------------------- ring header */
/* Device->host ordered log ring: device atomically bumps widx; host reads
 * records [ridx, widx) after a stream-ordered copy, then advances ridx.
 * Replaces the reference's BPF ring buffer (nat44.c:294-298). */
typedef struct bng_ring_header {
  uint32_t widx;     /* device atomic write index (monotonic, wraps mod 2^32) */
  uint32_t dropped;  /* records lost to a full ring                           */
  uint32_t capacity; /* power of two                                          */
  uint32_t _pad;
} bng_ring_header;  /* 16 B */

/* ------------------------------------------------- HA session export */
/* Compact NAT-session record for HA snapshot/delta sync (round-1
 * VERDICT task 3; ref pkg/ha/sync.go:25-815 replicates session state so
 * failover keeps NAT bindings).  Exported host-side from the session
 * table blob; imported on the standby by sess_import_kernel, which
 * recreates session + reverse (+ EIM when flags bit0) exactly as the
 * egress create path would. */
typedef struct bng_sess_export {
  uint32_t src_ip;    /* network order, as in bng_nat_tuple */
  uint32_t dst_ip;
  uint16_t src_port;  /* network order */
  uint16_t dst_port;
  uint8_t  protocol;
  uint8_t  state;
  uint8_t  is_hairpin;
  uint8_t  flags;     /* bit0: also restore the EIM mapping */
  uint32_t nat_ip;
  uint16_t nat_port;  /* network order, as in bng_nat_session */
  uint16_t eim_port;  /* HOST order, as in bng_eim_entry */
  uint64_t created;
  uint64_t last_seen;
  uint64_t _pad;
} bng_sess_export;  /* 48 B */

/* -------------------------------------------- persistent-service control */
/* SPSC doorbell between the host and the device-resident DHCP service
 * kernel (the persistent-kernel latency path: the service waves own
 * their CU permanently, so a saturating data flood cannot starve the
 * DHCP slice the way it starves a freshly launched kernel).  Lives in
 * PINNED HOST memory: host writes head/run/now, device writes tail.
 * No reference analog — kernel XDP gets this for free by running in
 * the NIC IRQ path; this is the MI355X equivalent. */
typedef struct bng_svc_ctrl {
  uint32_t head;        /* host bumps after writing a request batch   */
  uint32_t tail;        /* device bumps after replies are visible     */
  uint32_t run;         /* host clears to stop the kernel             */
  uint32_t n_pkts;      /* packets in the current batch               */
  uint64_t now_sec;     /* host-maintained batch clock                */
  uint32_t stride;
  uint32_t idle_exit_k; /* idle polls (units of 1024) before self-exit
                           — the box-safety bound                     */
  uint64_t served;      /* device: total packets served               */
  uint64_t batches;     /* device: total batches served               */
  uint32_t exited;      /* device: set on kernel exit (host watches
                           this so stop() can never block on a dead
                           doorbell)                                  */
  uint8_t  _pad[12];
} bng_svc_ctrl;  /* 64 B */

#ifdef __cplusplus
}
#endif

#endif /* BNG_ABI_H */
