"""What the cross-spectral host rule is worth at the sizes test_gpu_csm_large.py runs on the device: the device gives the rule's
bits there, so the rule's distance from fp64 at 2048 serial fp32 terms a chain is a question for a box without a GPU.

1. q of csm_map_host at 545 (of 640, ragged, with gains), 1121 and 2048 mics -- csm_large.py's lists, bin 47, Hann, two blocks --
   against s^H C s in float64.
2. csm_invert_rule_host at 512 mics, loading 1e-2, against numpy.linalg.inv of the loaded matrix formed in float64."""
import numpy as np
import pytest

import csm_large as L
import csm_util as CU
from test_csm_invert_cpu import loaded, random_matrix

# Measured on this build's host rule with the seeds below, each asserted at 4 x (tests/test_csm_cpu.py's convention): the inputs
# are seeded, so only the compiler and libm can move a figure.
Q_LARGE_MEASURED = {"545_of_640": 3.41e-7, "1121": 4.65e-7, "2048": 1.07e-6}  # |q - s^H C s (float64)| over the largest |q| of the plane
INVERSE_512_MEASURED = 5.47e-8  # |G - numpy.linalg.inv(A)| over the largest entry of the inverse


@pytest.mark.parametrize("name", list(Q_LARGE_MEASURED))
def test_q_against_fp64_at_large_lists(pkg, name):
    """The list's own table, samples and gains (csm_large.shape), bin 47, Hann, two blocks; C as csm_accumulate_host gives it, s
    from csm_steer_host, both taken to float64; the error relative to the plane's largest |q|, as test_accuracy_against_fp64 has
    it.  Measured here: 3.41e-7 at 545 mics (21 pixels), 4.65e-7 at 1121 (11 pixels), 1.07e-6 at 2048 (11 pixels), asserted at
    4 x.  A dropped row at 2048 mics would move q by about 1 / 2048 = 5e-4 of its size."""
    sh = L.shape(pkg, name)
    Cm, n = pkg.csm_accumulate_host(sh.samples_of(L.N_BLOCKS), L.BINS, L.WINDOW, index=sh.index, gain=sh.gain_list(), n_blocks=L.N_BLOCKS)
    q = pkg.csm_map_host(Cm, n, sh.off, sh.frac, L.BINS, L.WINDOW, index=sh.index, want=("q",))["q"][0]
    s = CU.as_complex(pkg.csm_steer_host(sh.off, sh.frac, L.BINS, index=sh.index))[:, 0]
    q64 = np.einsum("pa,ab,pb->p", s, CU.as_complex(Cm)[0], np.conj(s), optimize=True).real
    worst = float(np.abs(q - q64).max() / np.abs(q64).max())
    print(name, sh.U, "q against fp64:", worst, "bound", 4 * Q_LARGE_MEASURED[name])
    assert worst <= 4 * Q_LARGE_MEASURED[name], worst


def test_inverse_against_fp64_at_512_mics(pkg):
    """One bin, C = X X^H of 1027 complex normal columns (test_csm_invert_cpu.random_matrix, seed 612), loading 1e-2.  Measured
    here: 5.47e-8 of the inverse's largest entry, asserted at 4 x."""
    U, n = 512, 2 * 512 + 3
    Cm = random_matrix(np.random.default_rng(612), 1, U, n)
    Gf, solved = pkg.csm_invert_rule_host(Cm, n, [16], loading=1e-2)
    assert solved.tolist() == [1]
    inv = np.linalg.inv(loaded(Cm, n, 1e-2))
    worst = float(np.abs(CU.as_complex(Gf) - inv).max() / np.abs(inv).max())
    print("inverse at 512 mics against fp64:", worst, "bound", 4 * INVERSE_512_MEASURED)
    assert worst <= 4 * INVERSE_512_MEASURED, worst
