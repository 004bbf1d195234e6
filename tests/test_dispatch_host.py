"""csrc/dispatch.h, the header that turns the path entries' run-time booleans and the flux entry's
angle count into the template arguments of the kernel they launch: a stand-alone program, built
with the host C++ compiler alone (the header includes no HIP), checks that the constants handed
to the callable are the run-time values in argument order, that the callable runs exactly once,
and the contract for an integer outside the range."""
from pathlib import Path
import re
import shutil
import subprocess

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pylbl_amd" / "csrc"

PROGRAM = r"""
#include <cstdio>
#include "dispatch.h"

// What a kernel's template arguments would be: compile-time constants, so a swapped pair or a
// constant that is not one does not compile or is reported here.
template <int K, bool A, bool B>
struct Seen { static constexpr int k = K; static constexpr bool a = A, b = B; };

int main()
{
    int failures = 0, cases = 0;
    for (int bits = 0; bits < 8; ++bits)
    {
        const bool a = bits & 1, b = bits & 2, c = bits & 4;
        int calls = 0;
        lbl::dispatch([&](auto x, auto y, auto z) {
            using First = Seen<0, x.value, y.value>;
            using Second = Seen<0, y.value, z.value>;
            calls += 1;
            if (First::a != a || First::b != b || Second::a != b || Second::b != c) failures += 1;
        }, a, b, c);
        if (calls != 1) failures += 1;
        cases += 1;
    }
    for (int k = -1; k <= 10; ++k)
    {
        for (int bits = 0; bits < 4; ++bits)
        {
            const bool a = bits & 1, b = bits & 2;
            int calls = 0;
            const bool called = lbl::dispatch_range<8>([&](auto n, auto x, auto y) {
                using Got = Seen<n.value, x.value, y.value>;
                calls += 1;
                if (Got::k != k || Got::a != a || Got::b != b) failures += 1;
            }, k, a, b);
            // Inside 1..8: once, and true.  Outside: never, and false -- the caller has checked
            // the value (lbl_path_flux_source refuses n_angles outside 1..8 before it dispatches).
            const bool inside = k >= 1 && k <= 8;
            if (called != inside || calls != (inside ? 1 : 0)) failures += 1;
            cases += 1;
        }
    }
    int none = 0;
    lbl::dispatch([&] { none += 1; });
    if (none != 1) failures += 1;
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures == 0 ? 0 : 1;
}
"""


def host_compiler():
    for name in ("c++", "g++", "clang++"):
        found = shutil.which(name)
        if found:
            return found
    raise RuntimeError("no host C++ compiler (c++, g++, clang++) on the PATH.")


def test_the_header_needs_no_hip():
    text = (CSRC / "dispatch.h").read_text()
    assert "#include <hip" not in text and "hipLaunch" not in text
    assert '#include "dispatch.h"' in (CSRC / "path_entry.inc").read_text()


def test_constants_equal_the_run_time_values_in_order(tmp_path):
    source = tmp_path / "dispatch_check.cpp"
    source.write_text(PROGRAM)
    program = tmp_path / "dispatch_check"
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(CSRC),
                    str(source), "-o", str(program)], check=True)
    done = subprocess.run([str(program)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    # 8 boolean triples, and -1..10 with two booleans.
    assert done.stdout.strip() == "%d cases, 0 failures" % (8 + 12*4)


@pytest.mark.parametrize("entry, launches", [
    ("path_entry.inc", 1), ("radiance_entry.inc", 3), ("flux_entry.inc", 1),
    ("jacobian_entry.inc", 1), ("solar_entry.inc", 2)])
def test_every_launch_of_a_templated_kernel_goes_through_the_dispatcher(entry, launches):
    """No entry names a template argument by hand: <true>, <false> or a digit."""
    text = (CSRC / entry).read_text()
    templated = re.findall(r"hipLaunchKernelGGL\(\(?(\w+)<([^>]*)>", text)
    assert len(templated) == launches, templated
    for kernel, arguments in templated:
        assert re.fullmatch(r"\w\.value(, \w\.value)*", arguments), (kernel, arguments)
    assert "launch_flux" not in text and "launch_solar" not in text
