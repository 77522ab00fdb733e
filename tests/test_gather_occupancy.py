"""The one-hot gathers of the flagship shape must fit FOUR waves per SIMD: at most 128 VGPRs (512 / 128) and no scratch.  At B = 65 536
the launch is then 1 024 resident workgroups, one unit per wave -- one round; four registers more and 256 of them go round the
grid-stride loop a second time, from cold (profiles/NOTES.md R7.9).  Reads the kernels' metadata out of the built object; no GPU."""
import os
import re
import subprocess
import tempfile

import pytest

HEADLINE = "_ZN3dir15gather_onehot_kILi4ELi4ELi16ELi26E"           # gather_onehot_k<4, 4, 16, 26, *, *, *, *>
PACKED = ("_ZN3dir20gather_packed_rows_kILi4ELi13E", "_ZN3dir20gather_packed_rows_kILi8ELi13E")   # gather_packed_rows_k<4 | 8, 13, *>


def _kernel_notes(obj):
    """-> {kernel symbol: {metadata key: value}} from the gfx950 code object inside a HIP host object (llvm-readelf --notes)."""
    from dir_amd import isa_check
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "dev.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True, capture_output=True)
        subprocess.run([isa_check.LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--input=" + fat, "--output=" + co], check=True, capture_output=True)
        text = subprocess.run([isa_check.LLVM + "/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n\s*- \.agpr_count:", text)[1:]:          # one list item per kernel; .agpr_count is its first key
        block = ".agpr_count:" + block
        kv = dict(re.findall(r"^\s*(\.[a-z_]+):\s*(\S+)\s*$", block, re.M))
        if ".name" in kv:
            kernels[kv[".name"]] = kv
    return kernels


@pytest.fixture(scope="module")
def notes(built_lib):
    import dir_amd
    obj = os.path.join(os.path.dirname(dir_amd.library_path()), "csrc", "_build", "embedding_bag.o")
    assert os.path.exists(obj), obj
    return _kernel_notes(obj)


def test_flagship_gathers_fit_four_waves_per_simd(notes):
    head = {k: v for k, v in notes.items() if k.startswith(HEADLINE)}
    packed = {k: v for k, v in notes.items() if k.startswith(PACKED)}
    # fm+out, fm, out x NT on / off x the predicated and the quad issue phase; the packed rows kernel x NT on / off x 4 and 8 lanes
    assert len(head) == 12, sorted(head)
    assert len(packed) == 4, sorted(packed)
    for name, kv in sorted({**head, **packed}.items()):
        print(name, kv[".vgpr_count"], kv[".sgpr_count"], kv[".private_segment_fixed_size"])
        assert int(kv[".vgpr_count"]) + int(kv.get(".agpr_count", 0)) <= 128, (name, kv[".vgpr_count"], kv.get(".agpr_count"))
        assert int(kv[".private_segment_fixed_size"]) == 0, (name, kv[".private_segment_fixed_size"])


def test_no_kernel_of_the_gather_object_uses_scratch(notes):
    """The headline fit has no slack (128 of 128, under build.py's flags for this file: no packed fp32 VALU), and other instantiations
    of the same template must not pay for its bound: nothing in embedding_bag.o may spill."""
    assert len(notes) > 400
    spilled = {k: v[".private_segment_fixed_size"] for k, v in notes.items() if int(v[".private_segment_fixed_size"]) != 0}
    assert spilled == {}, spilled
