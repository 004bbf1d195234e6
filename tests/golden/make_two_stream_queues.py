"""The engine calls of the two-stream products -- compute_solar_flux, compute_solar_flux_spectral,
compute_thermal_flux, compute_thermal_flux_linear, compute_thermal_flux_spectral,
compute_thermal_radiance -- and of compute_solar, case by case, as the recording stand-in of
tests/two_stream_queue_cases.py sees them: two_stream_queues.json, which
tests/test_two_stream_queues_host.py compares the working tree with.

The file records what the code did BEFORE a change of the host side.  Make it on the commit the
change starts from, in a worktree that has the cases modules and this script copied in, and carry
the file over unchanged:
    git worktree add <scratch>/parent <parent commit>
    cp tests/two_stream_queue_cases.py tests/thermal_radiance_cases.py <scratch>/parent/tests/
    cp tests/golden/make_two_stream_queues.py <scratch>/parent/tests/golden/
    (cd <scratch>/parent && python tests/golden/make_two_stream_queues.py <here>/tests/golden)
Needs no GPU and no built library.
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    from tests import two_stream_queue_cases
    target = os.path.join(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(
        os.path.abspath(__file__)), "two_stream_queues.json")
    with tempfile.TemporaryDirectory() as directory:
        records = two_stream_queue_cases.run_cases(directory)
    with open(target, "w") as out:
        json.dump(records, out, indent=0, sort_keys=False)
        out.write("\n")
    calls = sum(len(record["log"]) for record in records.values())
    print(target, len(records), "cases", calls, "calls", os.path.getsize(target), "bytes")
