// staging.h — the one staging layer of the host-pointer flavours (`*_f64`): device copies of the inputs, the `_dev` entry, copies of the
// outputs back (not installed).  A call site registers every buffer once, with its size, and the address of the device pointer it wants:
//     Staging S(h, Staging::SCRATCH, "kl_terms");
//     S.in(&dK, K, m * n * nb); ... S.out(&dcx, cx, n * nb); ...
//     int rc = S.commit();                                  // places the buffers, fills the pointers, queues the uploads; -2 on failure
//     if (rc) return rc;
//     return S.finish(ddp_kl_terms_f64_dev(h, ..., dK, ..., dcx, ...));
// Two storage modes:
//   SCRATCH  carves the handle's scratch (ddp_scratch: grown on demand, kept by the handle, no allocation per call).  Only for entries
//            whose `_dev` callee does not use the scratch itself.
//   OWNED    one block of its own, freed when the Staging goes out of scope — after a stream synchronisation, on every way out.  For the
//            drivers (ilqg, the slot scheduler, ilqgkl) and every ddp_user_* entry: their callees carve the scratch themselves.
// Every buffer starts on a 256-byte boundary in both modes.
#pragma once
#include <string.h>
#include <vector>
#include "ddp_internal.h"

struct Staging {
    enum Mode { SCRATCH, OWNED };
    struct Buf { void *slot, *dev; const void *src; void *dst; size_t bytes; };      // slot: the address of the caller's device pointer
    ddp_handle h;
    Mode mode;
    const char *entry;                                           // names the entry in the OWNED-mode error message
    void *block = nullptr;                                       // OWNED: the allocation
    std::vector<Buf> bufs;
    Staging(ddp_handle h_, Mode mode_, const char *entry_) : h(h_), mode(mode_), entry(entry_) {}
    Staging(const Staging &) = delete;
    ~Staging() { if (block) { (void)hipStreamSynchronize(h->stream); (void)hipFree(block); } }

    // in: uploaded; a null source gives a null device pointer and no storage
    template <class T> void in(const T **slot, const T *host, size_t count) { *slot = nullptr; if (host) add(slot, host, nullptr, count * sizeof(T)); }
    // out: downloaded by finish(); a null destination gives a null device pointer and no storage
    template <class T> void out(T **slot, T *host, size_t count) { *slot = nullptr; if (host) add(slot, nullptr, host, count * sizeof(T)); }
    // out_or_temp: device storage always (the callee writes it whatever the caller wants), downloaded only if the host pointer is non-null
    template <class T> void out_or_temp(T **slot, T *host, size_t count) { add(slot, nullptr, host, count * sizeof(T)); }
    // inout: uploaded and downloaded; null gives a null device pointer and no storage
    template <class T> void inout(T **slot, T *host, size_t count) { *slot = nullptr; if (host) add(slot, host, host, count * sizeof(T)); }

    static size_t al(size_t b) { return (b + 255) & ~(size_t)255; }
    int commit()
    {
        const int rc = place();
        if (rc && mode == OWNED) ddp_set_error("%s: device allocation / upload failed", entry);
        return rc;
    }
    // rc of the `_dev` call: non-zero is returned as it is and nothing is downloaded; else the downloads and a stream synchronisation
    int finish(int rc)
    {
        if (rc) return rc;
        for (auto &b : bufs)
            if (b.dst) DDP_HIP(hipMemcpyAsync(b.dst, b.dev, b.bytes, hipMemcpyDeviceToHost, h->stream));
        DDP_HIP(hipStreamSynchronize(h->stream));
        return 0;
    }

private:
    void add(void *slot, const void *src, void *dst, size_t bytes) { bufs.push_back({slot, nullptr, src, dst, bytes}); }
    int place()
    {
        size_t need = 0;
        for (auto &b : bufs) need += al(b.bytes);
        void *base;
        if (mode == OWNED) { DDP_HIP(hipMalloc(&block, need ? need : 256)); base = block; }
        else { const int rc = ddp_scratch(h, need, &base); if (rc) return rc; }
        size_t off = 0;
        for (auto &b : bufs) {
            b.dev = (char *)base + off;
            off += al(b.bytes);
            memcpy(b.slot, &b.dev, sizeof b.dev);                // (the slot is a pointer of the caller's type)
            if (b.src) DDP_HIP(hipMemcpyAsync(b.dev, b.src, b.bytes, hipMemcpyHostToDevice, h->stream));
        }
        return 0;
    }
};

// Q, R of *p as inputs of S; pd->Q, pd->R are the device pointers once S.commit() has run.  On its own: ddp_df_f64, which reads nothing else
// of the problem and makes no diagonal test.
static inline void stage_cost(Staging &S, const ddp_problem *p, ddp_problem *pd)
{
    const size_t n = p->n, m = p->m;
    S.in(&pd->Q, p->Q, n * n); S.in(&pd->R, p->R, m * m);
}

// A whole problem: the host test of cost_diag = 1, then A, Bm of the LQ kind, then Q, R; *pd is *p with the device pointers once S.commit()
// has run.  The caller holds a DiagVerified from here until its `_dev` call has returned: the staged Q, R need no second test, and their
// addresses recycle from call to call.
static inline int stage_problem(Staging &S, const ddp_problem *p, ddp_problem *pd)
{
    { const int rd_ = ddp_check_cost_diag_host(p); if (rd_) return rd_; }
    const size_t n = p->n, m = p->m, dc = (size_t)(p->dyn_tv ? p->N : 1) * (p->dyn_batched ? p->B : 1);
    *pd = *p;
    if (p->kind == DDP_PROBLEM_LQ) { S.in(&pd->A, p->A, n * n * dc); S.in(&pd->Bm, p->Bm, n * m * dc); }
    stage_cost(S, p, pd);
    return 0;
}
