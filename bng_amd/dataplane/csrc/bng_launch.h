/* bng_launch.h — the extern "C" launcher ABI: bng_kernels.hip defines these,
 * bng_ext.cpp calls them, and both include this header, so a definition that
 * disagrees with its prototype fails to compile in the kernel unit instead of
 * linking and corrupting device memory.  Table and batch pointers stay void*:
 * the extension hands over raw tensor storage. */
#ifndef BNG_LAUNCH_H
#define BNG_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bng_params.h"

extern "C" {

void bng_set_pkt_grid_cap(int blocks);
int bng_get_pkt_grid_cap(void);
void bng_launch_dhcp(void* data, const void* in_len, void* out_len,
    void* verdict, int n, int stride, const void* subs, uint32_t sub_mask,
    const void* pools, uint32_t n_pools, const void* cfg, void* stats,
    uint64_t now_sec, const void* now_ptr, hipStream_t s);
void bng_launch_dhcp_service(void* ctrl, void* req, const void* in_len,
    void* out_len, void* verdict, void* scratch, int n_slots, int n_blocks,
    void* ctrs, const void* subs, uint32_t sub_mask, const void* pools,
    uint32_t n_pools, const void* cfg, void* stats, hipStream_t s);
void bng_launch_nat44(void* data, const void* in_len, void* verdict, int n,
    int stride, int is_egress, void* sessions, uint32_t sess_mask,
    void* reverse, uint32_t rev_mask, void* eim, uint32_t eim_mask,
    void* subnat, uint32_t subnat_mask, const void* cfg, const void* hairpin,
    uint32_t n_hairpin, void* stats, void* log_ring, void* log_hdr,
    uint64_t now_ns, hipStream_t s);
void bng_launch_qos(void* data, const void* in_len, void* verdict, int n,
    int stride, int is_egress, void* table, uint32_t mask, void* stats,
    uint64_t now_ns, hipStream_t s);
void bng_launch_antispoof(void* data, const void* in_len, void* verdict,
    int n, int stride, const void* bindings, uint32_t bmask, const void* cfg,
    void* stats, void* ring, void* hdr, uint64_t now_ns, hipStream_t s);
void bng_launch_uplink(bng_uplink_params* P, hipStream_t s);
void bng_launch_downlink(bng_uplink_params* P, hipStream_t s);
void bng_launch_pkt_class(const void* data, const void* in_len, void* cls,
    int n, int stride, hipStream_t s);
void bng_launch_shard_owner(const void* data, const void* in_len, void* owner,
    int n, int stride, int n_shards, hipStream_t s);
void bng_launch_pppoe_decap(void* data, void* in_len, void* state, int n,
    int stride, const void* sess, void* stats, hipStream_t s);
void bng_launch_pppoe_encap(void* data, void* in_len, void* verdict,
    void* state, int n, int stride, const void* by_ip, uint32_t ip_mask,
    const void* sess, const void* scfg, void* stats, hipStream_t s);
void bng_launch_sub_upsert(void* t, uint32_t mask, const void* batch, int n,
    void* rc, hipStream_t s);
void bng_launch_sub_delete(void* t, uint32_t mask, const void* keys, int n,
    hipStream_t s);
void bng_launch_sess_import(void* sess, uint32_t sess_mask, void* rev,
    uint32_t rev_mask, void* eim, uint32_t eim_mask, const void* batch, int n,
    void* rc, hipStream_t s);
void bng_launch_subctx_upsert(void* t, uint32_t mask, const void* batch,
    int n, uint32_t um, void* rc, hipStream_t s);
void bng_launch_qos_upsert(void* t, uint32_t mask, const void* batch, int n,
    void* rc, hipStream_t s);
void bng_launch_binding_upsert(void* t, uint32_t mask, const void* batch,
    int n, void* rc, hipStream_t s);
void bng_launch_binding_delete(void* t, uint32_t mask, const void* keys,
    int n, hipStream_t s);
void bng_launch_nat_sweep(void* sessions, uint32_t n_slots, void* reverse,
    uint32_t rev_mask, void* subnat, uint32_t subnat_mask, void* eim,
    uint32_t eim_slots, uint64_t eim_to, uint64_t now_ns, uint64_t udp_to,
    uint64_t tcp_est_to, uint64_t tcp_tr_to, uint64_t icmp_to, void* stats,
    hipStream_t s);
void bng_launch_pppoe_sess_upsert(void* sess, void* by_ip, uint32_t ip_mask,
    const void* batch, int n, void* rc, hipStream_t s);
void bng_launch_pppoe_sess_delete(void* sess, void* by_ip, uint32_t ip_mask,
    const void* sids, int n, hipStream_t s);
void bng_set_acct_combine(int rounds);
int bng_get_acct_combine(void);
void bng_launch_acct_resolve(const void* data, const void* in_len,
    void* slot, int n, int stride, const void* table, uint32_t mask,
    hipStream_t s);
void bng_launch_acct_commit(void* table, uint32_t mask, const void* slot,
    const void* verdict, const void* out_len, int n, uint64_t now_ns,
    hipStream_t s);
void bng_launch_acct_downlink(const void* data, const void* in_len,
    const void* verdict, int n, int stride, void* table, uint32_t mask,
    uint64_t now_ns, hipStream_t s);
void bng_launch_acct_upsert(void* table, uint32_t mask, const void* ips,
    int n, int reset, void* rc, hipStream_t s);
void bng_launch_acct_read(void* table, uint32_t mask, const void* ips, int n,
    void* out, hipStream_t s);
void bng_launch_acct_delete(void* table, uint32_t mask, const void* ips,
    int n, void* out, hipStream_t s);
void bng_launch_wg_uplink(const void* data, const void* in_len, void* verdict,
    void* out_len, void* gate, const void* order_in, void* order_out, int n,
    int stride, const void* table, uint32_t mask, const void* cfg,
    void* stats, hipStream_t s);
void bng_launch_wg_downlink(const void* data, const void* in_len,
    void* verdict, void* gate, int n, int stride, const void* table,
    uint32_t mask, const void* cfg, void* stats, hipStream_t s);
void bng_launch_wg_upsert(void* table, uint32_t mask, const void* batch,
    int n, void* rc, hipStream_t s);
void bng_launch_wg_delete(void* table, uint32_t mask, const void* ips, int n,
    hipStream_t s);

} /* extern "C" */

#endif /* BNG_LAUNCH_H */
