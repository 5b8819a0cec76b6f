"""CPU: tools/spectrum_scan.py --model on a small SigMF capture written with gr_lora_amd/sigmf.py (tests/spectrum_cases.py's two
emitters, as ci16_le): the bands it prints are the capture's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import spectrum_cases as sc
from gr_lora_amd import iqformat, sigmf, spectrum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "spectrum_scan.py")
FULL_SCALE = 16000.0
N = 40000                 # both emitters are on from sample 11003


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    base = str(tmp_path_factory.mktemp("scan") / "two_emitters")
    x = sc.capture()[:N]
    sigmf.write_trace(base, x, sc.FS, 868.1e6, 868.1e6, 7, "4/8", sc.BANDWIDTH, 8, True, False, "", 1, datatype="ci16_le", full_scale=FULL_SCALE)
    return base, x


def _args(base):
    return [base, "--nfft", str(sc.NFFT), "--hop", str(sc.HOP), "--n-avg", str(sc.N_AVG), "--grid=%g:%d:%d" % (sc.GRID_OFFSET, sc.N_GRID, sc.BANDWIDTH),
            "--channels=%d:%d" % (sc.CHANNELS[0], sc.CHANNELS[-1]), "--model"]


def test_model_scan_prints_the_bands_of_the_capture(written):
    base, x = written
    out = subprocess.run([sys.executable, TOOL] + _args(base) + ["--json"], check=True, capture_output=True, text=True, cwd=ROOT).stdout
    got = json.loads(out.strip().splitlines()[-1])
    assert got["datatype"] == "ci16_le" and got["source"] == "model" and got["samp_rate"] == sc.FS
    assert got["rows"] == spectrum.output_rows(N, sc.NFFT, sc.HOP, sc.N_AVG) and len(got["bands"]) == len(sc.CHANNELS)
    # what the tool must have computed: the model on the file's items under the default conversion
    q = iqformat.quantize(x, "sc16", FULL_SCALE)
    _, _, band, first = spectrum.welch_rows(iqformat.to_cf32(q), sc.NFFT, sc.HOP, sc.N_AVG, bands=sc.bands())
    for b, rec in enumerate(got["bands"]):
        assert (rec["first_bin"], rec["n_bins"]) == sc.bands()[b]
        assert abs(rec["mean_dbfs"] - float(spectrum.to_dbfs(band[:, b].mean()))) < 1e-9
        assert abs(rec["max_dbfs"] - float(spectrum.to_dbfs(band[:, b].max()))) < 1e-9
    # and what that means: the emitters at their amplitudes (full scale 16000 of 32768), the idle channels far below
    ref = 20 * np.log10(FULL_SCALE / 32768.0)
    mx = [rec["max_dbfs"] for rec in got["bands"]]
    assert abs(mx[sc.STRONG] - ref) <= 0.5 and abs(mx[sc.WEAK] - (ref + 20 * np.log10(0.25))) <= 0.5
    assert all(mx[c] <= mx[sc.STRONG] - 25.0 for c in range(len(mx)) if c not in (sc.STRONG, sc.WEAK))


def test_table_output_and_explicit_bands(written, capsys):
    base, _ = written
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import spectrum_scan
    finally:
        sys.path.pop(0)
    assert spectrum_scan.main([base + ".sigmf-meta", "--nfft", "256", "--n-avg", "8", "--band=-462500:-337500", "--band=0:100000", "--model"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert "ci16_le" in lines[0] and "nfft 256 hop 128 n_avg 8" in lines[0] and "(model)" in lines[0]
    assert len(lines) == 4
    strong, idle = lines[2].split(), lines[3].split()
    assert float(strong[0]) == -462500.0 and float(strong[1]) == -337500.0 and int(strong[2]) == 16
    assert float(strong[4]) > -7.0 and float(idle[4]) < float(strong[4]) - 25.0 and float(strong[3]) <= float(strong[4])
