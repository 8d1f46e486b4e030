// The workspace layout of the iLQGkl driver (csrc/kl_workspace.h) run without a device: from address 0 it measures, from a base it
// places.  For every shape and every kind of call the pieces are 256-byte aligned, disjoint, start with the counter block at the base,
// fill the block without a gap up to the measured size, and the size is the sum the driver used to write out by hand (old_size).
// Prints one line per case and "ok"; exit status 1 on the first failure.  tests/test_user_kl_cpu.py builds and runs it.
#include <algorithm>
#include <cstdio>
#include <vector>
#include "kl_workspace.h"

static size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

// the size as the driver summed it before the layout was one function
static size_t old_size(const KlWorkIn &w)
{
    const size_t n = w.n, m = w.m, N = w.N, B = w.B, NB = N * B, P2 = (n + m) * (n + m);
    const size_t hc = w.family ? (w.const_hessian && !w.hrep ? B : NB) : N, fxc = N * (w.fx_batched ? B : 1);
    size_t bytes = 0;
    bytes += w.fx_own ? al(n * n * fxc * 8) + al(n * m * fxc * 8) : 0;
    bytes += w.hrep ? al(n * n * B * 8) + al(n * m * B * 8) + al(m * m * B * 8) : 0;
    bytes += al(n * NB * 8) + al(m * NB * 8);                                                              // cx, cu
    bytes += al(n * n * hc * 8) + al(n * m * hc * 8) + al(m * m * hc * 8);                                 // cxx, cxu, cuu
    bytes += al(n * NB * 8) + al(m * NB * 8) + al(n * n * NB * 8) + al(m * n * NB * 8) + al(m * m * NB * 8);   // the KL terms
    bytes += al(m * NB * 8) + al(m * NB * 8);                                                              // k, zeros
    bytes += al(P2 * NB * 8) + al(NB * 8) + al(B * 8) + al(B * 8) + al(n * B * 8);                         // sigmanew, kldiv, klmean, csum, x0[:,1]
    bytes += al(3 * B * 8) + 4 * al(B * 8) + 6 * al(B * 4) + al(B * 4) + 256;                              // dual state, sum(cost0), diverge, counters
    return bytes;
}

struct Piece { const char *name; const void *p; size_t bytes; bool want = true; };

static std::vector<Piece> pieces(const KlWork &W, const KlWorkIn &w)
{
    const size_t n = w.n, m = w.m, N = w.N, B = w.B, NB = N * B;
    const size_t hc = w.family ? (w.const_hessian && !w.hrep ? B : NB) : N, fxc = N * (w.fx_batched ? B : 1);
    const ddp_kl_dual &s = W.dual.s;
    return {{"counter", W.counter, 256},
            {"cx", W.dv.cx, n * NB * 8}, {"cu", W.dv.cu, m * NB * 8}, {"cxx", W.dv.cxx, n * n * hc * 8}, {"cxu", W.dv.cxu, n * m * hc * 8},
            {"cuu", W.dv.cuu, m * m * hc * 8}, {"fxw", W.dv.fxw, n * n * fxc * 8, w.fx_own}, {"fuw", W.dv.fuw, n * m * fxc * 8, w.fx_own},
            {"hxx", W.dv.hxx, n * n * B * 8, w.hrep}, {"hxu", W.dv.hxu, n * m * B * 8, w.hrep}, {"huu", W.dv.huu, m * m * B * 8, w.hrep},
            {"kl cx", W.kt.cx, n * NB * 8}, {"kl cu", W.kt.cu, m * NB * 8}, {"kl cxx", W.kt.cxx, n * n * NB * 8},
            {"kl cxu", W.kt.cxu, m * n * NB * 8}, {"kl cuu", W.kt.cuu, m * m * NB * 8},
            {"etab", W.dual.etab_own, 3 * B * 8}, {"eta", s.eta, B * 8}, {"del", s.del, B * 8}, {"divergence", s.divergence, B * 8},
            {"satisfied", s.satisfied, B * 4}, {"status", s.status, B * 4}, {"live", s.live, B * 4}, {"pend", s.pend, B * 4},
            {"iters", s.iters, B * 4}, {"nback", s.nback, B * 4}, {"diverge", W.dual.div, B * 4}, {"klmean", W.dual.klm, B * 8},
            {"k", W.k, m * NB * 8}, {"kzero", W.kzero, m * NB * 8}, {"sigmanew", W.sig, (n + m) * (n + m) * NB * 8}, {"kldiv", W.kld, NB * 8},
            {"csum", W.cs, B * 8}, {"x0c", W.x0c, n * B * 8}, {"c0buf", W.c0buf, B * 8}};
}

static int check(const KlWorkIn &w)
{
    KlWork M, W;
    const size_t size = M.carve(Carver(), w);
    const uintptr_t base = (uintptr_t)0x7f3a00000000;
    const size_t end = W.carve(Carver((void *)base), w);
    printf("n=%zu m=%zu N=%zu B=%zu family=%d fx_own=%d fx_batched=%d const_hessian=%d hrep=%d: %zu bytes\n", w.n, w.m, w.N, w.B, w.family,
           w.fx_own, w.fx_batched, w.const_hessian, w.hrep, size);
#define FAIL(...) do { printf("FAILED: " __VA_ARGS__); printf("\n"); return 1; } while (0)
    if (size != old_size(w)) FAIL("measured %zu, the hand-written sum gives %zu", size, old_size(w));
    if (end != base + size) FAIL("placing ends at +%zu, measuring at %zu", end - base, size);
    std::vector<Piece> ps = pieces(W, w);
    if ((uintptr_t)ps[0].p != base) FAIL("the counter block is not first");
    for (const Piece &q : ps)
        if ((q.p != nullptr) != q.want) FAIL("%s is %s", q.name, q.p ? "placed" : "missing");
    ps.erase(std::remove_if(ps.begin(), ps.end(), [](const Piece &q) { return !q.p; }), ps.end());
    std::sort(ps.begin(), ps.end(), [](const Piece &a, const Piece &b) { return (uintptr_t)a.p < (uintptr_t)b.p; });
    uintptr_t at = base;
    for (const Piece &q : ps) {
        const uintptr_t p = (uintptr_t)q.p;
        if (p & 255) FAIL("%s is not 256-byte aligned", q.name);
        if (p < at) FAIL("%s overlaps the piece before it", q.name);
        if (p > at) FAIL("a gap of %zu bytes before %s", (size_t)(p - at), q.name);
        at = p + al(q.bytes);
    }
    if (at != base + size) FAIL("the pieces end at +%zu, the block at %zu", (size_t)(at - base), size);
    return 0;
}

int main()
{
    const size_t shapes[5][2] = {{4, 1}, {10, 2}, {32, 8}, {40, 20}, {64, 32}}, NBs[2][2] = {{7, 3}, {100, 16}};
    int cases = 0;
    for (const auto &sh : shapes)
        for (const auto &nb : NBs)
            for (int bits = 0; bits < 32; ++bits) {
                const KlWorkIn w = {sh[0], sh[1], nb[0], nb[1], (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0};
                // a family's dynamics are the driver's own and per trajectory; constant Hessians are a family's, hrep repeats constant ones
                if ((w.family && !(w.fx_own && w.fx_batched)) || (w.const_hessian && !w.family) || (w.hrep && !w.const_hessian)) continue;
                if (check(w)) return 1;
                ++cases;
            }
    printf("ok: %d cases\n", cases);
    return 0;
}
