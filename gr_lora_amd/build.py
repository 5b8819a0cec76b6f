"""Builds liblora_hip.so (HIP kernels + host runtime + C ABI) in-tree for gfx950."""
from __future__ import annotations

import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB = os.path.join(_HERE, "liblora_hip.so")
SOURCES = ["lora_kernels.hip", "lora_runtime.cpp", "lora_channelizer.hip", "lora_filterbank.hip", "lora_iq_unpack.hip", "lora_gateway.cpp", "lora_frame_check.cpp", "lora_tx.hip", "lora_link.hip", "lora_spectrum.hip", "lora_resampler.hip", "lora_conditioner.hip"]
DEPS = SOURCES + ["lora_device.h", "lora_stitch.hpp", "lora_walker2.inc.hip", "lora_walker3.inc.hip", "lora_team_demod.inc.hip", "lora_wave_demod.inc.hip", "lora_wave_decim.inc.hip", "lora_detect.inc.hip", "lora_soft.inc.hip", "lora_strict_sync.inc.hip", "lora_strict_resolve_lds.inc", "whitening_data.inc", "lora_mux_dev.h", "lora_iq.h", "lora_frame_check.h", "lora_link.h",
                  os.path.join("..", "..", "include", "lora_hip.h"), os.path.join("..", "..", "include", "lora_hip_channelizer.h"),
                  os.path.join("..", "..", "include", "lora_hip_filterbank.h"), os.path.join("..", "..", "include", "lora_hip_gateway.h"),
                  os.path.join("..", "..", "include", "lora_hip_tx.h"), os.path.join("..", "..", "include", "lora_hip_link.h"),
                  os.path.join("..", "..", "include", "lora_hip_spectrum.h"), os.path.join("..", "..", "include", "lora_hip_resampler.h"),
                  os.path.join("..", "..", "include", "lora_hip_conditioner.h"), os.path.join("..", "..", "include", "lora_hip_soft.h")]


CODEGEN_FLAGS = ["-mllvm", "-greedy-reverse-local-assignment"]


def hipcc_path() -> str:
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in DEPS)


def build_library(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 -> gr_lora_amd/liblora_hip.so (cross-compiles without a GPU)."""
    if not force and not stale():
        return LIB
    # -greedy-reverse-local-assignment: the walker kernels run at the 128-VGPR limit with 40-180 registers spilled; where the
    # reloads land decides their speed (docs/LAB_NOTEBOOK.md 5.2), and this order measured +2.5 % at SF9, +0.5 % at SF11, neutral elsewhere
    cmd = [hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-x", "hip",
           "-Wall", "-Wno-unused-function"] + CODEGEN_FLAGS + os.environ.get("LORA_HIP_EXTRA_FLAGS", "").split() + ["-I", CSRC, "-o", LIB] + [os.path.join(CSRC, s) for s in SOURCES]
    if verbose:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    import sys
    print(build_library(force=True, verbose="-v" in sys.argv))
