"""The case tables of tests/test_gpu_pdsch_softbits.py and tests/test_gpu_chan_softbits.py keep the sizes they are for (no device needed): the integer
demodulator's 16-QAM and 64-QAM routines treat the last n % 4 symbols (16-bit soft bits) or n % 8 symbols (8-bit) by another rule than the rest, and only a size that
is no multiple of that group holds a grant path's front end to it.  A later edit of the sizes must not quietly remove that."""
import test_gpu_chan_softbits as U
import test_gpu_pdsch_softbits as P

# transmit diversity on 4 ports takes multiples of 4 only: there is no 16-bit tail to reach
NO_TAIL = {("txdiv_4_ports", False)}


def test_every_path_family_has_a_tail_at_both_widths():
    tails = set()
    for case in P.CASES:
        group, path, _, mods, llr8, gain, skip = case
        n = P.nof_re_of(case)
        for k, mod in enumerate(mods):
            if k != skip and P.has_tail(mod, llr8, n):
                assert n % P.GROUP[llr8] != 0
                tails.add((group, P.family(path), llr8, mod))
                tails.add(("path", path, llr8, mod))
    families = {P.family(path) for path in P.PATHS}
    assert families == {"one_port", "txdiv_2_ports", "txdiv_4_ports", "mimo"}
    for llr8 in (False, True):
        for mod in (2, 3):
            for group in ("plain", "csi", "sf"):
                for fam in families:
                    if (fam, llr8) in NO_TAIL or (group == "sf" and fam == "txdiv_4_ports"):  # (the _sf forms: one case per family of calls, the 2-port one)
                        continue
                    assert (group, fam, llr8, mod) in tails, (group, fam, llr8, mod)
            for path in P.PATHS:  # every path of the plain calls on its own, not only its family
                if (P.family(path), llr8) not in NO_TAIL:
                    assert ("path", path, llr8, mod) in tails, (path, llr8, mod)


def test_the_4_port_exception_is_what_it_says():
    for case in P.CASES:
        if P.family(case[1]) == "txdiv_4_ports":
            assert P.nof_re_of(case) % 4 == 0 and (case[2] is None or case[2] % 8 == 4), case


def test_saturation_and_store_width_cases_are_there():
    """one 8-bit QPSK case with the receive gain per path family; QPSK at unit gain, BPSK and 256-QAM somewhere"""
    sat = {P.family(path) for _, path, _, mods, llr8, gain, _ in P.CASES if llr8 and gain and set(mods) == {1}}
    assert sat == {"one_port", "txdiv_2_ports", "txdiv_4_ports", "mimo"}
    assert all((2 * P.nof_re_of(c)) % 16 for c in P.CASES if c[5])  # QPSK: a tail of 2 n % 16 values
    assert {0, 1, 4} <= {m for _, _, _, mods, _, gain, _ in P.CASES if not gain for m in mods}
    assert any(skip is not None and P.nof_re_of(c) % 2 for c in P.CASES for skip in [c[6]])


def test_sf_cells_are_off_the_group_of_8():
    for path, cell in P.SF_PATHS.items():
        n = P.PM.indices(P.sf_cell(cell)).size
        assert P.sf_count_is_off_the_group(path, n) and n % 8 != 0 and n % 4 != 0, (path, n)


def test_pusch_has_8bit_grants_with_a_tail():
    """a PUSCH grant has 12 L_prb x columns symbols: a multiple of 4 always, of 8 unless L_prb x columns is odd"""
    plain = {name for name, counts in U.SINGLE if counts == (0, 0, 0)}
    tti = {name for name, _, _ in U.TTI}
    for mod in (2, 3):
        names = [n for n, g in U.GRANTS.items() if g[5] == mod and g[7] and (12 * g[4] * (2 * (g[1] - 1) - g[2])) % 8 == 4]
        assert any(n in plain for n in names) and any(n in tti for n in names), mod
