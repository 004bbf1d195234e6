"""CPU-only check of the gfx950 code object inside liblbl_amd.so: run_solve_kernel publishes a
sweep's pedestals (64-bit sc1 stores) and flags (global_atomic_or) before the 32-bit count that
announces them (global_store_dword), and its bin totals before the count of chunks that have left
(global_atomic_add), only if the wave waits for its vector-memory operations in between
(s_waitcnt vmcnt(0)).  A workgroup-scope fence lowers to an LDS wait, which another CU cannot
observe.  Reads the disassembly the way scripts/checks/kernel_registers.sh reads the notes."""
import os
from pathlib import Path
import re
import shutil
import subprocess

import pytest

LLVM = Path("/opt/rocm/lib/llvm/bin")
SOLVE = "_ZN3lbl16run_solve_kernel"


def _library():
    if os.environ.get("PYLBL_AMD_LIBRARY"):
        return Path(os.environ["PYLBL_AMD_LIBRARY"]).resolve()
    from pylbl_amd import build
    return build.build()


def _tool(name):
    path = LLVM / name
    if path.exists():
        return str(path)
    found = shutil.which(name)
    if found is None:
        pytest.fail(f"{name} not found: the ROCm LLVM tools are needed to read the code object")
    return found


@pytest.fixture(scope="module")
def disassembly(tmp_path_factory):
    work = tmp_path_factory.mktemp("code_object")
    fatbin, co = work / "fatbin", work / "co"
    subprocess.run([_tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fatbin}",
                    str(_library()), str(work / "unused.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fatbin}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    listing = subprocess.run([_tool("llvm-objdump"), "-d", "--mcpu=gfx950", str(co)], check=True,
                             capture_output=True, text=True).stdout
    return listing


def _functions(listing):
    """{symbol: [instruction text, ...]} in address order."""
    functions, name = {}, None
    for line in listing.splitlines():
        head = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if head:
            name = head.group(1)
            functions[name] = []
        elif name is not None and line.startswith("\t"):
            functions[name].append(line.split("//")[0].strip())
    return functions


def _unordered_publishes(body):
    """Count stores / exit adds with a data store or flag atomic before them that no
    s_waitcnt vmcnt(0) has waited for, in address order."""
    bad, pending = [], None
    for index, text in enumerate(body):
        mnemonic = text.split()[0] if text else ""
        if mnemonic in ("global_store_dwordx2", "global_atomic_or"):
            pending = (index, text)
        elif mnemonic == "s_waitcnt" and re.search(r"\bvmcnt\(0\)", text):
            pending = None
        elif mnemonic in ("global_store_dword", "global_atomic_add") and pending is not None:
            bad.append(f"{pending[1]!r} (#{pending[0]}) -> {text!r} (#{index})")
    return bad


def test_unordered_publishes_are_recognised():
    """The checker itself: the parent's sweep hand-over (an LDS wait only) is rejected, the
    same with vmcnt(0) in between is accepted."""
    parent = ["global_store_dwordx2 v[22:23], v[26:27], off sc1",
              "global_atomic_or v3, v45, s[16:17]",
              "s_waitcnt lgkmcnt(0)",
              "global_store_dword v3, v18, s[68:69] sc1"]
    assert len(_unordered_publishes(parent)) == 1
    fixed = parent[:3] + ["s_waitcnt vmcnt(0)"] + parent[3:]
    assert _unordered_publishes(fixed) == []
    exit_add = ["global_store_dwordx2 v[2:3], v[6:7], off sc1",
                "s_waitcnt lgkmcnt(0)",
                "global_atomic_add v2, v2, v3, s[22:23] offset:32 sc0"]
    assert len(_unordered_publishes(exit_add)) == 1
    assert _unordered_publishes(exit_add[:1] + ["s_waitcnt vmcnt(0) lgkmcnt(0)"] + exit_add[1:]) == []
    # (the serial chain's 64-bit float adds are not the exit count)
    assert _unordered_publishes(["global_store_dwordx2 v[4:5], v[2:3], off",
                                 "global_atomic_add_f64 v[62:63], v[40:41], off"]) == []


def test_run_solve_waits_before_every_count(disassembly):
    functions = _functions(disassembly)
    solves = {name: body for name, body in functions.items() if name.startswith(SOLVE)}
    # run_solve_kernel<true> (windows of at most 64 slots) and <false>
    assert len(solves) == 2, sorted(solves)
    for name, body in solves.items():
        mnemonics = [text.split()[0] for text in body if text]
        # what the check is about is there: the sweep's count, the exit count, the flags
        assert "global_store_dword" in mnemonics, name
        assert "global_atomic_add" in mnemonics, name
        assert "global_atomic_or" in mnemonics, name
        bad = _unordered_publishes(body)
        assert bad == [], f"{name}: count published before its data:\n" + "\n".join(bad)
