"""The case table of tests/test_gpu_small_partition.py is complete: every kernel that xmris_amd/csrc launches through
xm_launch_items, or whose grid it sizes with xm_resident_blocks, has a small-partition case there.  Runs without a GPU: it
reads the launchers' source."""
import glob
import os
import re

import test_gpu_small_partition as cases

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xmris_amd", "csrc")
SITE = re.compile(r"\bxm_(launch_items|resident_blocks)\s*\(")
KERNEL = re.compile(r"\bk_\w+")
COMMENT = re.compile(r"//[^\n]*|/\*.*?\*/", re.S)  # a comment may speak of either function without calling it


def call_sites():
    """[(file:line, "launch_items" | "resident_blocks", kernel or None)]: the kernel is the first k_... name of the
    statement, as in xm_launch_items(res, k_x<...>, ...) and xm_resident_blocks(res, (k_x<S, PT>), ...)."""
    sites = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.inc"))):
        text = COMMENT.sub(lambda c: re.sub(r"[^\n]", " ", c.group(0)), open(path).read())  # (the line numbers stay)
        for m in SITE.finditer(text):
            name = KERNEL.search(text, m.end(), text.index(";", m.end()))
            where = f"{os.path.basename(path)}:{text.count(chr(10), 0, m.start()) + 1}"
            sites.append((where, m.group(1), name.group(0) if name else None))
    return sites


def test_every_call_site_names_a_kernel():
    sites = call_sites()
    assert len(sites) >= 20 and all(k for _, _, k in sites), [s for s in sites if not s[2]]


def test_every_persistent_kernel_has_a_small_partition_case():
    found = {}
    for where, _, kernel in call_sites():
        found.setdefault(kernel, []).append(where)
    missing = {k: v for k, v in found.items() if k not in cases.CASES}
    assert not missing, f"persistent kernels without a case in tests/test_gpu_small_partition.py: {missing}"
    stale = sorted(set(cases.CASES) - set(found))
    assert not stale, f"cases for kernels that no launcher sizes by its stream: {stale}"


def test_the_table_says_how_each_grid_is_sized():
    ticket = {k for _, how, k in call_sites() if how == "launch_items"}
    for kernel, c in cases.CASES.items():
        assert c["grid"] == ("ticket" if kernel in ticket else "stride"), kernel
        assert c["factor"] >= 1 and (c["nt"] is None or c["nt"] % 64 == 0), kernel
        for name in c["tests"]:
            assert callable(getattr(cases, name, None)), (kernel, name)
