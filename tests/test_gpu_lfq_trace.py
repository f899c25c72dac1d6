"""sage_hip_lfq's tracing half — windows_kernel, the two radix sorts and page_keys_kernel, spectrum_setup_kernel, count_kernel /
fill_kernel, the stable sort of the contribution list, row_reduce_kernel — on feature maps of 1, 2, 4, 5, 8 and 9 pages,
against a reading that knows no page and no sort of the windows (tests/lfq_trace_bruteforce.py).

One lfq / lfq_im call with debug=True per world of tests/lfq_trace_worlds.py.  What the worlds are built to reach — a matched
window in every page, both sides of the seams, a spectrum over three or more pages, the shared min_rt a tolerance away, the
last row of the last slot, cells whose sum shows the order of their additions — is asserted by tests/test_lfq_trace_cpu.py,
which also holds the pruned matcher used here equal to the exhaustive one; the worlds come from fixed seeds.  Exact:
n_windows, n_contributions, the grid keys, every matrix as uint64 bits.  Integration outputs are not compared, but for p1,
whose device results go through test_gpu_lfq_integration.assert_second_reading as it stands.

Wall time per test on the MI355X (building the world and the brute force included):
p1 0.68 s, p2 0.08 s, p4 0.10 s, p5 0.12 s, p8 0.14 s, p9 0.14 s.  tests/test_gpu_lfq_integration.py, unchanged since the parent
commit, in the same run: 5.0 s for its 30 tests, the slowest 0.40 s.  p1 is above that: nearly all of its time is the second
reading of its 816 grids (about 0.5 s on the host), not the trace; its spectra are already at the 100 the worlds start from."""
import numpy as np
import pytest

import lfq_trace_bruteforce as B
import lfq_trace_worlds as W
from sage_amd.api import LfqSettings, lfq, lfq_im
from test_gpu_lfq_integration import assert_second_reading

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worlds(gpu_required):
    return W.world   # (built once: lfq_trace_worlds keeps them)


def pages_of(wd, key):
    w = wd["windows"]
    mine = (w["peptide"] == key[0]) & (w["decoy"] == key[2]) & ((w["charge"] == key[1]) | wd["spec"]["combine"])
    return np.unique(wd["page"][mine]).tolist()


@pytest.mark.parametrize("name", W.NAMES)
def test_trace_matches_brute_force(worlds, name):
    wd = worlds(name)
    sp = wd["spec"]
    grids, n_matches, _ = W.brute(wd, prune=True)
    st = LfqSettings(ppm_tolerance=sp["ppm"], mobility_pct_tolerance=sp["pct"], combine_charge_states=sp["combine"])
    dev = (lfq_im if sp["im"] else lfq)(wd["f"], None, wd["art"], wd["pq"], wd["al"], wd["batches"], wd["carbon"], wd["sulfur"], st,
                                        sp["charge"], debug=True)
    assert dev.n_windows == W.WINDOWS[name]
    assert dev.n_contributions == n_matches > 5000
    keys = [(int(p), int(z), bool(d)) for p, z, d in zip(dev.peptide_idx, dev.charge, dev.decoy)]
    assert keys == sorted(grids), "grid keys"
    assert keys[-1] == (wd["pmax"], 0 if sp["combine"] else sp["charge"][1], True), "the last grid slot"
    want = np.stack([grids[k] for k in keys])
    assert dev.matrix.shape == want.shape == (len(keys), wd["n_files"] * 3, 100)
    differ = dev.matrix.view(np.uint64) != want.view(np.uint64)
    if differ.any():
        i, row, col = (int(x[0]) for x in np.nonzero(differ))
        raise AssertionError(f"{name}: {int(differ.sum())} cells differ, the first in grid {keys[i]} (windows in pages {pages_of(wd, keys[i])}) "
                             f"row {row} bin {col}: device {dev.matrix[i, row, col]!r}, brute force {want[i, row, col]!r}")
    if name == "p1":
        rows = B.select(wd["f"]["peptide_idx"], wd["f"]["label"], wd["pq"], st.peptide_q_value)
        reference_file = {int(p): int(f) for p, f in zip(wd["f"]["peptide_idx"][rows], wd["f"]["file_id"][rows])}
        assert_second_reading(wd["db"], dev, reference_file, W.settings_of(name))
