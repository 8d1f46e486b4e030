"""The table of rollout calls that pins which kernel ddp_forward_pass_f64_dev launches (csrc/forward_pass.hip, fp_choose), shared by
tests/test_gpu_forward_contract.py (each call on the device: ddp_last_kernel(h, 1) and the rollouts themselves) and
tests/test_fp_choice.py (the library's choice through its debug hook, no GPU).  No tests here."""
PIPE4, PIPE, DPP, ROW = "forward_pipe4_kernel", "forward_pipe_kernel", "forward_dpp_kernel", "forward_row_kernel"
MID, BIG, GRP = "forward_mid_kernel", "forward_big_kernel", "forward_pass_kernel"


def row(fam, n, m, want, B=7, na=3, dyn="", pol=True, lims=False, full=True, mis=(), Ns=(5,), **env):
    """fam: "lq" | "pend"; dyn: "" shared LTI, "F" shared LTV, "f" / "Ff" per trajectory; full: full Q and R with cost_diag = 0, else
    diagonal ones with cost_diag = 1; mis: the operands placed 8 bytes into their allocation (of K k u x A B); Ns: the horizons the
    call is made at; env: DDP_* switches by their name without the prefix"""
    return dict(fam=fam, n=n, m=m, want=want, B=B, na=na, dyn=dyn, pol=pol, lims=lims, full=full, mis=tuple(mis), Ns=tuple(Ns),
                env={("DDP_" + k): v for k, v in env.items()})


def lq102(want, **kw):                        # the (10, 2) call the pipeline takes unless a row says otherwise
    kw.setdefault("full", False)
    return row("lq", 10, 2, want, **kw)


def pend(B, na, **kw):
    kw.setdefault("Ns", (15, 16, 17))
    kw.setdefault("full", False)
    return row("pend", 4, 1, kw.pop("want", DPP), B=B, na=na, **kw)


S63, S15, SP = (63, 64, 65), (15, 16, 17), (7, 8, 9, 11, 12, 13)
TABLE = [
    # (10, 2), policy, no limits, diagonal cost, aligned operands: the pipeline up to 1 024 rollouts (forward_pass_pipe.hip; fp_choose, total <= 1024)
    lq102(PIPE4, Ns=(1, 2, 3) + SP), lq102(PIPE4, B=64, na=16, Ns=(12, 13)), lq102(DPP, B=205, na=5, Ns=(12, 13)),
    lq102(PIPE4, B=1024, na=1, Ns=(9,)), lq102(DPP, B=1025, na=1, Ns=(9,)),
    lq102(PIPE, dyn="F", Ns=(1, 2, 3) + SP), lq102(PIPE, dyn="Ff", Ns=SP), lq102(PIPE, dyn="f", Ns=SP),
    lq102(PIPE, dyn="F", B=64, na=16, Ns=(8, 9)), lq102(DPP, dyn="F", B=205, na=5, Ns=(8, 9)), lq102(DPP, dyn="Ff", B=205, na=5, Ns=(8,)),
    # ... and each single reason for which it declines
    lq102(DPP, pol=False, Ns=(1, 2, 3, 16)), lq102(DPP, lims=True, Ns=(1, 2, 3, 16)), lq102(DPP, full=True, Ns=S63), lq102(DPP, FORWARD_PIPE="0"),
    lq102(DPP, FORWARD_FUSE="0", Ns=S63), lq102(DPP, mis="K"), lq102(DPP, mis="k"), lq102(DPP, mis="u"), lq102(DPP, mis="x"),
    lq102(DPP, dyn="F", mis="A"), lq102(DPP, dyn="F", mis="B"), lq102(DPP, dyn="Ff", lims=True, full=True, Ns=(2, 17)),
    lq102(PIPE4, mis="AB", Ns=(9,)),            # (time-invariant dynamics are not fetched in 16-byte pieces: no reason to decline)
    lq102(PIPE4, B=128, na=16, Ns=(12,), FORWARD_PIPE="1"), lq102(PIPE, Ns=SP, FORWARD_PIPE="2"), lq102(PIPE, B=128, na=16, dyn="F", Ns=(8,), FORWARD_PIPE="1"),
    # the variants of the 16-lane-row kernel (launch_dpp: FAST, from fp_choose's `fast` and the alignment of u, k, K)
    lq102(DPP, FORWARD_FAST="0", FORWARD_PIPE="0"), lq102(DPP, lims=True, FORWARD_FAST="0"), lq102(DPP, mis="uk", lims=True), lq102(DPP, mis="Kkux", Ns=(3, 16)),
    lq102(DPP, dyn="f", pol=False, lims=True, full=True),
    # LQ shapes a padded 16-lane row holds (forward_pass_row.hip, ddp_launch_forward_row)
    row("lq", 1, 1, ROW, Ns=(1, 2, 3) + S63), row("lq", 4, 1, ROW, dyn="F", Ns=S63), row("lq", 6, 3, ROW, lims=True, Ns=S63),
    row("lq", 12, 4, ROW, dyn="Ff", lims=True, Ns=S63), row("lq", 13, 2, ROW, pol=False, Ns=S63), row("lq", 14, 1, ROW, dyn="f", Ns=S63),
    row("lq", 14, 2, ROW, dyn="F", lims=True, Ns=S63), row("lq", 8, 2, ROW, pol=False, lims=True, Ns=(1, 64)), row("lq", 9, 2, ROW, mis="Kkux", Ns=(3, 33)),
    # what no row holds, up to n = 32: one wave per rollout (forward_pass_big.hip, forward_mid_kernel)
    row("lq", 13, 3, MID, Ns=(1, 2, 3) + S63), row("lq", 14, 4, MID, lims=True, Ns=S63), row("lq", 15, 1, MID, dyn="F", Ns=S63),
    row("lq", 16, 8, MID, dyn="Ff", lims=True, Ns=S63), row("lq", 17, 1, MID, pol=False, Ns=S63), row("lq", 24, 4, MID, dyn="f", Ns=S63),
    row("lq", 25, 8, MID, lims=True, Ns=S63), row("lq", 32, 8, MID, dyn="F", Ns=S63), row("lq", 3, 5, MID, lims=True, Ns=S63),
    row("lq", 24, 4, MID, mis="KkuxAB", dyn="F", Ns=(4, 33)),
    *[row("lq", n, m, BIG, Ns=(1, 2, 3, 64) if n == 13 else (64, 65), FORWARD_MID="0", **kw) for n, m, kw in (
        (13, 3, {}), (14, 4, dict(lims=True)), (15, 1, dict(dyn="F")), (16, 8, dict(dyn="Ff", lims=True)), (17, 1, dict(pol=False)),
        (24, 4, dict(dyn="f")), (25, 8, dict(lims=True)), (32, 8, dict(dyn="F")), (3, 5, dict(lims=True)))],
    # 32 < n <= 64: forward_big_kernel with cost_mid_kernel<48> / <64>; full Q and R reach the last rows and columns of the padding
    row("lq", 33, 1, BIG, Ns=(1, 2, 3) + S63), row("lq", 40, 5, BIG, dyn="F", lims=True, Ns=S63), row("lq", 47, 8, BIG, dyn="Ff", Ns=S63),
    row("lq", 48, 6, BIG, lims=True, Ns=S63), row("lq", 49, 1, BIG, dyn="f", Ns=S63), row("lq", 63, 8, BIG, dyn="F", lims=True, Ns=S63),
    row("lq", 64, 1, BIG, pol=False, lims=True, Ns=S63), row("lq", 64, 7, BIG, dyn="Ff", lims=True, Ns=S63),
    row("lq", 48, 8, BIG, pol=False, Ns=(1, 64)), row("lq", 64, 8, BIG, dyn="F", lims=True, Ns=(1, 2, 3) + S63, FORWARD64="0"),
    row("lq", 48, 6, BIG, lims=True, Ns=(64, 65), FORWARD_MID="0"), row("lq", 40, 5, BIG, mis="KkuxAB", dyn="F", Ns=(4, 33)),
    # (64, 8): forward_big64_kernel (1, 2 or 4 step sizes of a trajectory per wave) reports the family's name
    *[row("lq", 64, 8, BIG, B=5, na=na, pol=pol, lims=(na % 2 == 1), dyn=("F" if na in (2, 5) else ""), Ns=((1, 2, 3) if na == 3 else ()) + S15)
      for na in (1, 2, 3, 5, 16) for pol in (True, False)],
    # DDP_FORWARD=group: the run-time-sized group-of-lanes kernel, the five instantiations of launch_fp
    row("lq", 10, 2, GRP, Ns=(1, 2, 3, 16), FORWARD="group"), row("lq", 4, 1, GRP, dyn="F", lims=True, FORWARD="group"),
    row("lq", 6, 3, GRP, dyn="Ff", FORWARD="group"), row("lq", 9, 2, GRP, pol=False, lims=True, FORWARD="group"),
    row("lq", 16, 3, GRP, dyn="f", lims=True, FORWARD="group"), row("lq", 17, 3, GRP, dyn="F", FORWARD="group"),
    row("lq", 32, 8, GRP, lims=True, Ns=(9,), FORWARD="group"), row("lq", 10, 2, GRP, full=False, mis="Kkux", FORWARD="group"),
    # DDP_FORWARD=b: the large-state launcher first
    row("lq", 10, 2, MID, Ns=(3, 64), FORWARD="b"), row("lq", 20, 3, MID, lims=True, dyn="F", Ns=(64,), FORWARD="b"),
    # pendcart (forward_pass_dpp.hip): element-wise / chunked streams at 3 584 rollouts, the lane kernel from 12 288
    pend(7, 3, Ns=(1, 2, 3) + S15), pend(7, 3, pol=False, lims=True, Ns=(1, 2, 3) + S15), pend(5, 2, lims=True, full=True),
    pend(3583, 1, Ns=(16, 17)), pend(512, 7, Ns=(16, 17)), pend(3583, 1, pol=False, lims=True, Ns=(17,)), pend(224, 16, lims=True, Ns=(15, 24)),
    pend(1117, 11, Ns=(17,)), pend(768, 16, Ns=(16, 17)), pend(1117, 11, lims=True, pol=False, Ns=(24,)), pend(768, 16, lims=True, Ns=(15,)),
    pend(12288, 1, pol=False, Ns=(3,)),
    pend(7, 3, lims=True, FORWARD_LANE="1"), pend(70, 3, pol=False, Ns=(1, 2, 3, 17), FORWARD_LANE="1"), pend(768, 16, Ns=(17,), FORWARD_LANE="0"),
    pend(7, 3, lims=True, PEND_CHUNK="1"), pend(512, 7, Ns=(17,), PEND_CHUNK="0"), pend(7, 3, lims=True, FORWARD_PEND="0"),
    pend(7, 3, pol=False, FORWARD_PEND="0", FORWARD_FUSE="0"), pend(7, 3, lims=True, FORWARD_FUSE="0"), pend(70, 3, FORWARD_FUSE="0", FORWARD_LANE="1"),
    pend(7, 3, lims=True, want=GRP, Ns=(1, 2, 3, 16), FORWARD="group"), pend(7, 3, pol=False, want=GRP, FORWARD="group"),
]


def _id(r):
    return "%s_n%d_m%d_B%dx%d_%s_%s%s%s%s_%s" % (r["fam"], r["n"], r["m"], r["B"], r["na"], r["dyn"] or "lti", "pol" if r["pol"] else "open",
                                                "_lims" if r["lims"] else "", "_full" if r["full"] else "_diag",
                                                ("_mis" + "".join(r["mis"])) if r["mis"] else "",
                                                "_".join("%s=%s" % (k[4:], v) for k, v in sorted(r["env"].items())) or "default")
