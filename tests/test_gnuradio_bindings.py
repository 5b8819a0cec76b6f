"""SURVEY 8(f) N3, the rest of the GNU Radio packaging around the drop-in decoder block:

* shim/gnuradio/python/bindings/decoder_hip_python.cc -- the pybind11 binding that takes the place of
  python/bindings/decoder_python.cc (:36-66): compiled UNCHANGED against pybind11 and the stand-in runtime of
  tests/mock_gnuradio, imported, its signature checked; on a GPU box the block is constructed from Python with the
  reference's argument names and decodes the known-answer capture under a scheduler loop;
* shim/gnuradio/CMakeLists.txt -- the overlay build whose gnuradio-lora target links lora_hip instead of liquid
  (lib/CMakeLists.txt:41-42): configured and built with cmake in its LORA_HIP_MOCK_GNURADIO mode;
* shim/gnuradio/grc/lora_receiver_hip.block.yml -- the GRC definition: same block id, parameters, make template and
  callbacks as grc/lora_receiver.block.yml:3-88 (checked against a summary committed here, and field by field against the
  reference's own file as tests/golden/grc_lora_receiver_block.json records it)."""
import importlib.util
import json
import os
import shutil
import subprocess
import sys
import sysconfig
import textwrap

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "shim", "gnuradio")

# the module entry a gr-lora build gets from python/bindings/python_bindings.cc (:45-67): here it first registers the
# stand-in base classes (the real one imports gnuradio.gr for that) and adds a scheduler loop for the test
MODULE_MAIN = textwrap.dedent(r'''
    #include <pybind11/pybind11.h>
    #include <pybind11/numpy.h>
    #include <pybind11/stl.h>
    #include <lora/decoder.h>
    namespace py = pybind11;
    void bind_decoder(py::module &m);
    PYBIND11_MODULE(lora_python_mock, m) {
        py::class_<gr::basic_block, std::shared_ptr<gr::basic_block>>(m, "basic_block");
        py::class_<gr::block, gr::basic_block, std::shared_ptr<gr::block>>(m, "block");
        py::class_<gr::sync_block, gr::block, std::shared_ptr<gr::sync_block>>(m, "sync_block")
            .def_readonly("mock_output_multiple", &gr::sync_block::mock_output_multiple)
            .def_readonly("mock_ports", &gr::sync_block::mock_ports);
        bind_decoder(m);
        m.def("run_to_completion", [](std::shared_ptr<gr::lora::decoder> blk, py::array_t<std::complex<float>, py::array::c_style> iq) {
            const gr_complex *x = iq.data();
            const long long n = (long long)iq.size(), m = blk->mock_output_multiple;
            long long pos = 0;
            while (n - pos >= m) {   // offers multiples of the output multiple, advances by what the block consumed
                const int offer = (int)(((n - pos < 16 * m ? n - pos : 16 * m) / m) * m);
                gr_vector_const_void_star in{x + pos};
                gr_vector_void_star out;
                const long long before = blk->mock_consumed;
                if (blk->work(offer, in, out) != 0) throw std::runtime_error("work() returned non-zero");
                if (blk->mock_consumed == before) break;
                pos += blk->mock_consumed - before;
            }
            blk->stop();
            std::vector<py::bytes> frames;
            for (auto &p : blk->mock_published)
                if (p.first == "frames") frames.emplace_back(static_cast<const char *>(pmt::blob_data(p.second)), pmt::blob_length(p.second));
            return frames;
        });
    }
''')


def _build_module(tmp_path):
    import pybind11
    from gr_lora_amd import build
    build.build_library()
    main = tmp_path / "module_main.cc"
    main.write_text(MODULE_MAIN)
    out = tmp_path / ("lora_python_mock" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-fvisibility=hidden",
                           "-I", pybind11.get_include(), "-I", sysconfig.get_paths()["include"],
                           "-I", os.path.join(ROOT, "tests", "mock_gnuradio"), "-I", os.path.join(ROOT, "include"), "-I", SHIM,
                           str(main), os.path.join(SHIM, "python", "bindings", "decoder_hip_python.cc"), os.path.join(SHIM, "decoder_impl.cc"),
                           "-o", str(out), "-L", os.path.join(ROOT, "gr_lora_amd"), "-llora_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "gr_lora_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    spec = importlib.util.spec_from_file_location("lora_python_mock", str(out))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_decoder_signature(tmp_path):
    mod = _build_module(tmp_path)
    d = mod.decoder
    assert issubclass(d, mod.sync_block) and issubclass(d, mod.block) and issubclass(d, mod.basic_block)
    doc = d.__init__.__doc__
    # argument names and order of the reference binding (decoder_python.cc:40-48)
    names = ["samp_rate", "bandwidth", "sf", "implicit", "cr", "crc", "reduced_rate", "disable_drift_correction"]
    pos = [doc.index(n + ":") for n in names]
    assert pos == sorted(pos)
    assert "set_sf" in dir(d) and "set_samp_rate" in dir(d)
    with pytest.raises(TypeError):   # no defaults: all eight arguments are required, as upstream
        d(1e6, 125000, 7)


@pytest.mark.gpu
def test_pybind_block_decodes_known_answer(tmp_path, capfd):
    mod = _build_module(tmp_path)
    blk = mod.decoder(samp_rate=1e6, bandwidth=125000, sf=7, implicit=False, cr=4, crc=True, reduced_rate=False, disable_drift_correction=False)
    assert blk.mock_output_multiple == 2 * 1024 and blk.mock_ports == ["frames", "control"]
    blk.set_sf(8)   # warn-only (decoder_impl.cc:905-909)
    iq = np.fromfile(os.path.join(ROOT, "tests", "golden", "sf7_cr4_deadbeef_x2.cf32"), dtype=np.complex64)
    frames = mod.run_to_completion(blk, iq)
    assert [f[15:].hex() for f in frames] == ["049040deadbeef700d"] * 2


def test_cmake_overlay_target_builds(tmp_path):
    if shutil.which("cmake") is None:
        pytest.skip("cmake not installed")
    from gr_lora_amd import build
    build.build_library()
    bdir = tmp_path / "b"
    gen = ["-G", "Ninja"] if shutil.which("ninja") else []
    subprocess.check_call(["cmake", "-S", SHIM, "-B", str(bdir), "-DLORA_HIP_MOCK_GNURADIO=ON", "-DLORA_HIP_ROOT=" + ROOT] + gen,
                          stdout=subprocess.DEVNULL)
    subprocess.check_call(["cmake", "--build", str(bdir)], stdout=subprocess.DEVNULL)
    libs = [f for f in os.listdir(bdir) if f.startswith("libgnuradio-lora")]
    assert libs, os.listdir(bdir)
    needed = subprocess.run(["readelf", "-d", str(bdir / libs[0])], capture_output=True, text=True).stdout
    assert "liblora_hip.so" in needed and "liquid" not in needed
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", str(bdir / libs[0])], capture_output=True, text=True).stdout
    assert "gr::lora::decoder::make(float, unsigned int, unsigned char, bool, unsigned char, bool, bool, bool)" in syms


def test_cmake_overlay_names_the_upstream_parts():
    txt = open(os.path.join(SHIM, "CMakeLists.txt")).read()
    for part in ("decoder_impl.cc", "decoder_hip_python.cc", "lora_receiver_hip.block.yml", "gnuradio::gnuradio-runtime", "lora_hip"):
        assert part in txt
    body = "\n".join(l for l in txt.split("\n") if not l.lstrip().startswith("#"))
    assert "liquid" not in body


GRC_PARAMS = [  # (id, dtype, default) in the order of grc/lora_receiver.block.yml:7-70
    ("samp_rate", "float", 1e6), ("center_freq", "float", 868e6), ("channel_list", "float_vector", [868.1e6]), ("bandwidth", "int", 125000),
    ("sf", "int", 7), ("implicit", "bool", False), ("cr", "enum", None), ("crc", "bool", True), ("reduced_rate", "bool", False),
    ("conj", "bool", False), ("decimation", "int", 1), ("disable_channelization", "bool", False), ("disable_drift_correction", "bool", False)]


def _norm(d):
    d = dict(d)
    d.pop("documentation", None); d.pop("flags", None)
    t = dict(d["templates"]); t["make"] = " ".join(t["make"].split()); d["templates"] = t
    return d


def test_grc_block_definition():
    y = yaml.safe_load(open(os.path.join(SHIM, "grc", "lora_receiver_hip.block.yml")))
    assert y["id"] == "lora_lora_receiver" and y["file_format"] == 1
    got = [(p["id"], p["dtype"], p.get("default")) for p in y["parameters"]]
    num = lambda c: float(c) if isinstance(c, str) else [num(e) for e in c] if isinstance(c, list) else c   # PyYAML reads 1e6 as a string
    assert [(a, b, num(c)) for a, b, c in got] == GRC_PARAMS
    cr = y["parameters"][6]
    assert cr["options"] == [4, 3, 2, 1] and cr["option_labels"] == ["4/8", "4/7", "4/6", "4/5"]
    make = " ".join(y["templates"]["make"].split())
    args = [a.strip() for a in make[make.index("(") + 1:make.rindex(")")].split(",")]
    assert make.startswith("lora.lora_receiver(") and args == ["${%s}" % p[0] for p in GRC_PARAMS]   # python/lora_receiver.py:30
    assert y["templates"]["callbacks"] == ["set_center_freq(${center_freq})", "set_sf(${sf})"]
    assert y["inputs"] == [{"domain": "stream", "dtype": "complex"}]
    assert y["outputs"] == [{"domain": "message", "id": "frames", "optional": True}]
    # the whole definition, field by field: the reference's grc/lora_receiver.block.yml as _norm() reads it
    with open(os.path.join(ROOT, "tests", "golden", "grc_lora_receiver_block.json")) as f:
        assert _norm(y) == json.load(f)
