"""Lean posing, without a GPU: the kernels that now pose their own queries keep the residency they had (registers, LDS,
no scratch) and the lean posing kernel spills nothing -- read from the compiler's resource-usage remarks for gfx950."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "multi-view-registration_amd"


@pytest.fixture(scope="module")
def usage(built, tmp_path_factory):
    out = {}
    tmp = tmp_path_factory.mktemp("lean_pose")
    for name in ("mvr_grid.hip", "mvr_reduce.hip", "mvr_index.hip"):
        src = os.path.join(ROOT, PKG, "csrc", name)
        r = subprocess.run([built.HIPCC] + built.HIP_FLAGS + ["-x", "hip", "-c", src, "-o", str(tmp / (name + ".o")),
                            "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        for b in re.split(r"(?=remark: Function Name: )", r.stdout)[1:]:
            num = lambda key: int(re.search(key + r": (\d+)", b).group(1))
            fn = re.search(r"Function Name: (\S+)", b).group(1)
            demangled = subprocess.run(["c++filt", fn], stdout=subprocess.PIPE, text=True).stdout.strip() or fn
            out[demangled] = dict(vgprs=num(r"VGPRs"), lds=num(r"LDS Size \[bytes/block\]"), waves=num(r"Occupancy \[waves/SIMD\]"),
                                  scratch=num(r"ScratchSize \[bytes/lane\]"))
    return out


def _one(usage, pattern):
    hits = [(n, u) for n, u in usage.items() if re.search(pattern, n)]
    assert len(hits) == 1, (pattern, [n for n, _ in hits])
    return hits[0][1]


# waves/SIMD of the hot kernels before they posed their own queries: none may drop
@pytest.mark.parametrize("pattern,waves,vgprs,lds", [
    (r"nn_grid_kernel<false, true>", 8, 64, 10240),
    (r"nn_grid_kernel<false, false>", 8, 64, None),
    (r"nn_grid_tail_kernel<false>", 5, None, None),
    (r"nn_grid_wide_kernel<false>", 7, None, None),
    (r"accept_moments2_batch_kernel", 4, 128, None),
])
def test_hot_kernels_keep_their_residency(usage, pattern, waves, vgprs, lds):
    u = _one(usage, pattern)
    print(pattern, u)
    assert u["waves"] >= waves, u
    assert u["scratch"] == 0, u
    if vgprs is not None:
        assert u["vgprs"] <= vgprs, u
    if lds is not None:
        assert u["lds"] <= lds, u


def test_lean_posing_kernel_uses_no_scratch(usage):
    u = _one(usage, r"pose_grid_lean_kernel")
    assert u["scratch"] == 0, u
