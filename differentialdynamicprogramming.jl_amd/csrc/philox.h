// philox.h — the one definition of the library's random normals: included by sample.hip (ddp_normal_fill) and handed as text to hiprtc
// for ddp_user_sample (build.py writes build/philox_text.h from this file, as it does for boxqp_dev.h).  Plain integer and double
// arithmetic, no #include of its own.
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of
//     (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)),    M0 = 0xD2511F53, M1 = 0xCD9E8D57,
// the key bumped by (0x9E3779B9, 0xBB67AE85) between rounds.  One call per (step, sample, trajectory, pair):
//     counter = (i, sample0 + s, traj0 + b, q),   key = (seed_lo, seed_hi)
// and from its four words one pair of normals by Box-Muller:
//     k1 = (r0 >> 5) 2^26 + (r1 >> 6),  k2 = (r2 >> 5) 2^26 + (r3 >> 6)        (53 bits each)
//     u1 = (k1 + 1) 2^-53 in (0, 1],    u2 = k2 2^-53 in [0, 1)
//     xi[2q] = sqrt(-2 log u1) cos(2 pi u2),   xi[2q + 1] = sqrt(-2 log u1) sin(2 pi u2)   (dropped when 2q + 1 == m)
// Nothing depends on the launch geometry, on S, B or the chunking: a call that passes its own sample0 / traj0 draws its slice of the
// full array, bit for bit.
#pragma once

__device__ __forceinline__ void ddp_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                                  unsigned (&r)[4])
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// the pair q of normals of (step i, sample s, trajectory b), s and b absolute (sample0, traj0 added by the caller)
__device__ __forceinline__ void ddp_normal_pair(unsigned seed_lo, unsigned seed_hi, int i, int s, int b, int q, double &z0, double &z1)
{
    unsigned r[4];
    ddp_philox4x32_10((unsigned)i, (unsigned)s, (unsigned)b, (unsigned)q, seed_lo, seed_hi, r);
    const unsigned long long k1 = ((unsigned long long)(r[0] >> 5) << 26) + (r[1] >> 6), k2 = ((unsigned long long)(r[2] >> 5) << 26) + (r[3] >> 6);
    const double u1 = (double)(k1 + 1) * 0x1p-53, u2 = (double)k2 * 0x1p-53;
    const double rho = sqrt(-2.0 * log(u1)), ang = 6.283185307179586 * u2;
    z0 = rho * cos(ang);
    z1 = rho * sin(ang);
}
