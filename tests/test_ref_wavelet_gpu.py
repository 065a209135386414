"""The reference's own wavelet tree programs, compiled as they lie against the drop-in layer (tools/ref_bind_check.py --install-ref-tests
-> oracle/_ref/ref_wavelet_test, ref_waveletfm; built where the reference's sources are, skipped where they are absent), run on the GPU:
nvbio-test/wavelet_test.cu must pass its text and known-rank checks on this layout, examples/waveletfm/waveletfm.cu must print the BWT,
the primary and one occurrence for every suffix of its protein text, as tests/wavelet_reference.py computes them."""
import os
import re
import subprocess

import pytest

from nvbio_amd import alphabet
from tests import wavelet_cases as WC
from tests import wavelet_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")


def run(name, args, timeout=300):
    exe = os.path.join(REF, name)
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/%s not built (needs /root/reference in the build container)" % name)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout)
    return r.returncode, (r.stdout + r.stderr).replace("\r", "\n")


def test_reference_wavelet_test_passes():
    rc, text = run("ref_wavelet_test", [])
    assert rc == 0, text[-2000:]
    assert "error" not in text, text[-2000:]
    assert "wavelet test... done" in text, text[-2000:]


def test_reference_waveletfm_prints_the_bwt_and_one_occurrence_per_suffix():
    rc, text = run("ref_waveletfm", [])
    assert rc == 0, text[-2000:]
    sym = alphabet.encode(WC.PROTEIN_TEXT)
    sa = R.suffix_array(sym, 8)
    bwt, primary = R.bwt(sym, 8, sa)
    assert "bwt: %s (primary %u)" % (alphabet.decode(bwt), primary) in text, text[-2000:]
    ranks = re.findall(r"rank\(([A-Z]+)\): (\d+)", text)
    assert ranks == [(WC.PROTEIN_TEXT[i:], "1") for i in range(len(WC.PROTEIN_TEXT))], ranks
    assert "waveletfm... done" in text
