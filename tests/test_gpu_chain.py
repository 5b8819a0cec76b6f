"""GPU: the device's five copies of the integer decode chain - what happens to a symbol's bin on its way to the frame bytes: reduced-rate
rounding, gray word, block de-interleaver, de-shuffle, de-whitening, Hamming(8,4) or data bits, header parse, frame assembly - on ARBITRARY symbols.

Frames from synth.encode_shifts are valid codewords: of the 256-entry Hamming table they read 16 entries, their parity bits never disagree, no header
carries a bit error, the CR field is never 0 or 5-7, the reduced-rate rounding only sees multiples of 4.  The frames here are crafted
(tests/chain_model.py: craft_frame, case_sets) - payloads of uniformly drawn words, every one-bit and two-bit error on every header codeword, every
value of the header fields, symbols one to three bins off the reduced-rate grid, the longest payloads - and modulated on a clean signal, where the
demodulators return every symbol exactly; they reach the chain through lora_hip_decode_device like any capture.  Required of every stream, in every
family of kernels that holds a copy of the chain ("The integer decode chain"):

* the frames equal the oracle's byte for byte, loratap header included, and the header positions are equal;
* the frames equal chain_model.chain_decode's - the plain-Python definition that tests/test_chain_model.py holds the oracle to on the same streams;
* the kernel that ran is the family's (lora_hip_walker_kernel_name, with or without _wide / _half / _skip / _d2 / _d4), and the payload pass decoded
  packets exactly where it is meant to.

No tolerance anywhere: bytes and integer positions.

Input rules (chain_model's docstring has the reasons): the full-rate word 1 << (sf - 1) - shift 0, an unshifted upchirp - is never drawn at random
and is sent in the `top_word` cases only, to demodulators 1 and 2 (the gradient demodulator's answer to it is an accident of rounding; at decimation
2 / 4 to demodulator 1 only: demodulator 2 pins its bin to 0, and fine_sync, fed that bin, moves the symbol clock by a sample - half a bin there); the residue
cases that send bin N - 1 in a header or reduced-rate symbol go to demodulators 1 and 2 as well; a frame whose first header symbol the gradient
demodulator cannot decide when its window sits one sample off (Frame.gradient_safe, computed in float64 from the symbols sent) goes to demodulators
1 and 2 only; every frame sends exactly the symbols its header - as decoded under the carried CR - asks for, then silence."""
import concurrent.futures as cf
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import chain_model as M
from gr_lora_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORACLE = {}


def _render(cell, demod):
    """[(stream index, frames, iq)] of the streams of the cell that go to `demod`"""
    cfg = synth.TxConfig(**cell[1])
    return [(i, frames, M.render(frames, cfg)) for i, frames in M.streams_for(cell, demod)]


def _oracle(oracle_mod, cell, demod, rendered):
    """{stream index: [(frame, header position)]} from the oracle, once per (cell, demodulator) and process"""
    key = (cell[0], demod)
    if key not in _ORACLE:
        def one(item):
            o = oracle_mod.Oracle(**M.decoder_kwargs(cell[2], demod))
            o.run(item[2])
            return item[0], list(zip(o.frames(), o.frame_positions()))
        with cf.ThreadPoolExecutor(8) as ex:
            _ORACLE[key] = dict(ex.map(one, rendered))
    return _ORACLE[key]


def decode_cell(torch, cell, demod, rendered, flags=0, cycle=1):
    """the cell's streams in ONE lora_hip_decode_device call -> ({stream index: [(frame, header position)]}, kernel name, payload-pass packets, jobs);
    cycle > 1: that many copies of the list of streams (the same samples), every copy's output must be the first's"""
    from gr_lora_amd import capi
    iq = np.concatenate([r[2] for r in rendered])
    offs, pos = [], 0
    for r in rendered:
        offs.append(pos)
        pos += r[2].size
    lens = [r[2].size for r in rendered]
    dev = torch.from_numpy(iq.view(np.float32)).to("cuda:0")
    h = capi.Handle(flags=flags, **M.decoder_kwargs(cell[2], demod))
    h.decode_device(dev.data_ptr(), iq.size, offs * cycle, lens * cycle, torch.cuda.current_stream().cuda_stream)
    per = {}
    for blob, info in h.drain():
        per.setdefault(int(info.stream), []).append((bytes(blob), int(info.header_pos)))
    name, packets, jobs = h.kernel_name(), int(h.payload_pass()["packets"]), int(h.timing().jobs)
    h.close()
    n = len(rendered)
    out = {rendered[k][0]: per.get(k, []) for k in range(n)}
    for k in range(n, n * cycle):
        assert per.get(k, []) == per.get(k % n, []), (cell[0], demod, "copy", k)
    return out, name, packets, jobs


def check_cell(oracle_mod, cell, demod, rendered, got):
    want = _oracle(oracle_mod, cell, demod, rendered)
    for i, frames, _ in rendered:
        what = (cell[0], "stream", i, "demod", demod, [f.note for f in frames])
        assert len(want[i]) == len(frames), what + ("the oracle's frames", len(want[i]), len(frames))
        assert [g[0] for g in got[i]] == [w[0] for w in want[i]], what + ("frames against the oracle", [g[0][15:].hex() for g in got[i]], [w[0][15:].hex() for w in want[i]])
        assert [g[1] for g in got[i]] == [w[1] for w in want[i]], what + ("header positions against the oracle",)
        assert [g[0][15:] for g in got[i]] == M.expect(frames, cell[2], demod), what + ("frames against chain_decode",)


def run_family(torch, oracle_mod, family, sf, demod, kernel, payload_pass=False, flags=0, cycle=1, min_jobs=0, max_jobs=None):
    names = [n for n, d in M.families()[family] if d == demod and M.cell(n)[2]["sf"] == sf]
    assert names, (family, sf, demod)
    n_frames = 0
    for name in names:
        cell = M.cell(name)
        rendered = _render(cell, demod)
        if not rendered:
            continue
        got, kname, packets, jobs = decode_cell(torch, cell, demod, rendered, flags, cycle)
        want_kernel = kernel(cell) if callable(kernel) else kernel
        assert kname == want_kernel, (name, demod, kname, want_kernel)
        assert (packets > 0) == payload_pass, (name, demod, packets)
        assert jobs >= min_jobs and (max_jobs is None or jobs <= max_jobs), (name, jobs)
        check_cell(oracle_mod, cell, demod, rendered, got)
        n_frames += sum(len(r[1]) for r in rendered)
    assert n_frames > 0
    print(family, "SF%d" % sf, "demod", demod, len(names), "cells", n_frames, "frames")


def _cells_of(family):
    return sorted({(M.cell(n)[2]["sf"], d) for n, d in M.families()[family]})


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU: the HIP path has no CPU fallback")
    return torch


def _g(demod):
    return "_grad" if demod == 0 else ""


def _decim_of(cell):
    return {v: k for k, v in M.RATES.items()}[cell[2]["samp_rate"]]


@pytest.mark.gpu
@pytest.mark.parametrize("sf,demod", _cells_of("walker2_wide"))
def test_walker2_wide_builds(torch_cuda, oracle_mod, monkeypatch, sf, demod):
    """w2_post_symbol<true, false> and deinterleave_block_wave: no more jobs than CUs"""
    monkeypatch.setenv("LORA_HIP_DECOUPLED", "0")
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    run_family(torch_cuda, oracle_mod, "walker2_wide", sf, demod, "walker2_kernel_sf%d%s_wide" % (sf, _g(demod)), max_jobs=cus)


@pytest.mark.gpu
@pytest.mark.parametrize("sf,demod", _cells_of("walker2_two_per_cu"))
def test_walker2_two_per_cu_builds(torch_cuda, oracle_mod, monkeypatch, sf, demod):
    """the same chain in the builds that share a CU: more jobs than CUs - twenty copies of sixteen single-packet streams"""
    monkeypatch.setenv("LORA_HIP_DECOUPLED", "0")
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    run_family(torch_cuda, oracle_mod, "walker2_two_per_cu", sf, demod, "walker2_kernel_sf%d%s" % (sf, _g(demod)), cycle=-(-(cus + 64) // 16), min_jobs=cus + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("sf,demod", _cells_of("walker2_decim"))
def test_walker2_at_decimation_2_and_4(torch_cuda, oracle_mod, monkeypatch, sf, demod):
    """SF7 / SF8 with the words as bytes, SF9 as 16-bit fields (deinterleave_block_wave16: ppm = 9, and the reduced rate's ppm = 7), SF6 implicit"""
    monkeypatch.setenv("LORA_HIP_DECOUPLED", "0")
    run_family(torch_cuda, oracle_mod, "walker2_decim", sf, demod, lambda c: "walker2_kernel_sf%d_d%d%s" % (sf, _decim_of(c), _g(demod)))


@pytest.mark.gpu
@pytest.mark.parametrize("sf,demod", _cells_of("walker3"))
def test_walker3(torch_cuda, oracle_mod, monkeypatch, sf, demod):
    """w3_post_symbol from the fast replay round, the complete kernels (payload rounds in the walker)"""
    monkeypatch.setenv("LORA_HIP_DECOUPLED", "0")
    run_family(torch_cuda, oracle_mod, "walker3", sf, demod, "walker3_kernel_sf%d%s" % (sf, _g(demod)))


@pytest.mark.gpu
@pytest.mark.parametrize("sf,demod", _cells_of("walker3_trace"))
def test_walker3_general_replay_loop(torch_cuda, oracle_mod, monkeypatch, sf, demod):
    """w3_post_symbol from the general replay loop, which runs under tracing"""
    from gr_lora_amd import capi
    monkeypatch.setenv("LORA_HIP_DECOUPLED", "0")
    run_family(torch_cuda, oracle_mod, "walker3_trace", sf, demod, "walker3_kernel_sf%d%s" % (sf, _g(demod)), flags=capi.FLAG_TRACE)


@pytest.mark.gpu
@pytest.mark.parametrize("sf,demod", _cells_of("payload_pass"))
def test_payload_pass(torch_cuda, oracle_mod, monkeypatch, sf, demod):
    """payload_chain_kernel behind the header-only walkers: every payload through the pass, the header parse in the *_skip kernels, the carried CR
    and the spare header codewords through PayloadDesc"""
    monkeypatch.setenv("LORA_HIP_DECOUPLED", "1")
    run_family(torch_cuda, oracle_mod, "payload_pass", sf, demod, "walker%d_kernel_sf%d%s_skip" % (2 if sf <= 8 else 3, sf, _g(demod)), payload_pass=True)


@pytest.mark.gpu
@pytest.mark.parametrize("sf,demod", _cells_of("generic"))
def test_generic_walker(torch_cuda, oracle_mod, monkeypatch, sf, demod):
    """deinterleave_block / decode_header_bytes / decode_payload_bytes on thread 0 of the generic walker: LORA_HIP_NO_FAST=1 at SF7 and SF9, and SF10
    at decimation 4, which no fast family covers; the implicit header at SF7"""
    monkeypatch.setenv("LORA_HIP_DECOUPLED", "0")
    if sf != 10:
        monkeypatch.setenv("LORA_HIP_NO_FAST", "1")
    names = ("walker_kernel", "walker_kernel_f1", "walker_kernel_f0")
    seen = []

    def kernel(cell):
        from gr_lora_amd import capi
        h = capi.Handle(**M.decoder_kwargs(cell[2], demod))
        seen.append(h.kernel_name())
        h.close()
        return seen[-1]
    run_family(torch_cuda, oracle_mod, "generic", sf, demod, kernel)
    assert seen and all(s in names for s in seen), seen


# ---- walker3's half-size workgroups: LORA_HIP_W3_HALF is read once per process -----------------------------------------------------------------
def half_cells():
    return [(n, d) for n, d in M.families()["walker3_half"]]


def decode_half(torch):
    out = {}
    for name, demod in half_cells():
        cell = M.cell(name)
        rendered = _render(cell, demod)
        if rendered:
            out[(name, demod)] = decode_cell(torch, cell, demod, rendered)
    return out


@pytest.fixture(scope="module")
def half_runs(torch_cuda, tmp_path_factory):
    """every cell of the family decoded in ONE fresh process with LORA_HIP_W3_HALF=1"""
    assert "LORA_HIP_W3_HALF" not in os.environ
    out = str(tmp_path_factory.mktemp("chain_half") / "half.pkl")
    env = dict(os.environ, LORA_HIP_W3_HALF="1", LORA_HIP_DECOUPLED="0", PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    with open(out, "rb") as f:
        return pickle.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("sf,demod", _cells_of("walker3_half"))
def test_walker3_half_size_workgroups(half_runs, oracle_mod, sf, demod):
    n = 0
    for (name, d), (got, kname, packets, jobs) in half_runs.items():
        cell = M.cell(name)
        if d != demod or cell[2]["sf"] != sf:
            continue
        assert kname == "walker3_kernel_sf%d%s_half" % (sf, _g(demod)) and packets == 0, (name, kname, packets)
        check_cell(oracle_mod, cell, demod, _render(cell, demod), got)
        n += 1
    assert n > 0


def test_every_family_sees_every_header_error_pattern():
    """all 36 one-bit and two-bit patterns on at least one header codeword and every codeword index, in every family (on the demodulators 1 / 2 the
    gradient rule keeps nothing from; the walker2 SF7 cell carries all 180)"""
    for family, cells in M.families().items():
        if family == "walker2_two_per_cu":                             # (the same kernel source as the wide builds, built with another register budget)
            continue
        pats, idx = set(), set()
        for name, demod in cells:
            if name.startswith("header_bit_errors/") and demod == 2:
                for frames in M.cell(name)[3]:
                    i, m = frames[0].note[2:].split("^")
                    idx.add(int(i))
                    pats.add(int(m, 16))
        assert pats == set(M.PATTERNS) and idx == set(range(5)), (family, len(pats), idx)
    assert len(M.cell("header_bit_errors/sf7_cr4")[3]) == 180 and ("header_bit_errors/sf7_cr4", 2) in M.families()["walker2_wide"]


if __name__ == "__main__":   # the child process of half_runs
    import torch
    with open(sys.argv[1], "wb") as f:
        pickle.dump(decode_half(torch), f)
