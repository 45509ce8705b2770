"""The fused ray kernel's register budget, read from the built library's code-object metadata (runs without a GPU).

A scratch reload inside the software-pipelined decode waits, through the in-order vmcnt, for every gather load issued before it, so the
REF shape's kernel and config 5's must not spill VGPRs to scratch.  A library math call in the marcher (ocml's expm1f / log1pf) was once
enough to bring 4 spilled VGPRs and 8 more SGPR spills back; this catches the next such change at build time.
"""
import os
import re
import struct
import subprocess
import tempfile

import pytest

from real3dportrait_amd import _lib

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
REF = "_ZN3r3d13render_kernelILi3ELi3ELi2ELi1ELb0EEEvNS_10RenderArgsEi"      # render_kernel<3, 3, 2, 1, false>: the benchmarked frame
CFG5 = "_ZN3r3d13render_kernelILi6ELi6ELi2ELi1ELb0EEEvNS_10RenderArgsEi"     # render_kernel<6, 6, 2, 1, false>: BASELINE config 5


def _code_objects(blob):
    """The amdgcn ELF code objects embedded in a host shared library (the offload bundles of its .hip_fatbin section)."""
    out, i = [], 0
    while True:
        i = blob.find(b"\x7fELF\x02\x01", i + 1)
        if i < 0:
            return out
        if struct.unpack_from("<H", blob, i + 18)[0] != 0xE0:          # EM_AMDGPU
            continue
        shoff = struct.unpack_from("<Q", blob, i + 0x28)[0]
        shentsize, shnum = struct.unpack_from("<HH", blob, i + 0x3A)
        out.append(blob[i:i + shoff + shentsize * shnum])


def _kernel_metadata(lib_path):
    """{kernel symbol: {metadata key: value}} from the AMDGPU metadata notes of every code object of the library."""
    with open(lib_path, "rb") as f:
        blob = f.read()
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, co in enumerate(_code_objects(blob)):
            path = os.path.join(tmp, "co%d.o" % k)
            with open(path, "wb") as f:
                f.write(co)
            notes = subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in notes.splitlines():
                m = re.match(r"^(\s+)(- )?\.(\w+):\s+(\S+)\s*$", line)
                if not m:
                    continue
                indent = len(m.group(1)) + (2 if m.group(2) else 0)
                if indent != 4:                                    # a kernel's own keys (deeper: its arguments' keys, .name among them)
                    continue
                if m.group(2):                                     # "  - .agpr_count:" opens the next entry of amdhsa.kernels
                    cur = {}
                if cur is None:
                    continue
                cur[m.group(3)] = m.group(4)
                if m.group(3) == "name":
                    kernels[m.group(4)] = cur
    return kernels


@pytest.fixture(scope="module")
def meta():
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    return _kernel_metadata(_lib.LIB_PATH)


@pytest.mark.parametrize("sym", [REF, CFG5])
def test_render_kernel_does_not_spill_to_scratch(meta, sym):
    m = meta[sym]
    assert int(m["vgpr_spill_count"]) == 0, m
    assert int(m["private_segment_fixed_size"]) == 0, m


def test_ref_render_kernel_sgpr_spills(meta):
    # the count of the build before the library math calls (each spilled SGPR costs a v_writelane / v_readlane on the VALU the kernel is bound by)
    assert int(meta[REF]["sgpr_spill_count"]) <= 52, meta[REF]
