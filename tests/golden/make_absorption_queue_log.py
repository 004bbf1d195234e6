"""The engine calls of Spectroscopy.compute_absorption, case by case, as the recording stand-in of
tests/absorption_recorder.py sees them: absorption_queue_log.json, which
tests/test_absorption_queue_host.py compares the working tree with.

The file records what the code did BEFORE a change of the host side.  Make it on the commit the
change starts from, in a worktree that has tests/absorption_recorder.py and this script copied
in, and carry the file over unchanged:
    git worktree add <scratch>/parent <parent commit>
    cp tests/absorption_recorder.py <scratch>/parent/tests/
    cp tests/golden/make_absorption_queue_log.py <scratch>/parent/tests/golden/
    (cd <scratch>/parent && python tests/golden/make_absorption_queue_log.py <here>/tests/golden)
Needs no GPU and no built library.
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    from tests import absorption_recorder
    target = os.path.join(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(
        os.path.abspath(__file__)), "absorption_queue_log.json")
    with tempfile.TemporaryDirectory() as directory:
        records = absorption_recorder.run_cases(directory)
    with open(target, "w") as out:
        json.dump(records, out, indent=0, sort_keys=False)
        out.write("\n")
    calls = sum(len(record["log"]) for record in records.values())
    print(target, len(records), "cases", calls, "calls", os.path.getsize(target), "bytes")
