"""What ShardedLines.run does on the host, case by case and rank by rank, as the recording gloo ranks
of tests/sharded_lines_recorder.py see it: sharded_lines_log.json, which
tests/test_sharded_lines_log_host.py compares the working tree with.

The file records what the code did BEFORE a change of pylbl_amd/distributed.py.  Make it on the
commit the change starts from, in a worktree that has tests/sharded_lines_recorder.py and this
script copied in, and carry the file over unchanged:
    git worktree add <scratch>/parent <parent commit>
    cp tests/sharded_lines_recorder.py <scratch>/parent/tests/
    cp tests/golden/make_sharded_lines_log.py <scratch>/parent/tests/golden/
    (cd <scratch>/parent && python tests/golden/make_sharded_lines_log.py <here>/tests/golden)
Needs no GPU and no built library.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    from tests import sharded_lines_recorder
    target = os.path.join(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(
        os.path.abspath(__file__)), "sharded_lines_log.json")
    records = sharded_lines_recorder.run_cases()
    with open(target, "w") as out:
        json.dump(records, out, indent=0, sort_keys=False)
        out.write("\n")
    entries = sum(len(log) for record in records.values() for log in record.values())
    print(target, len(records), "cases", entries, "entries", os.path.getsize(target), "bytes")
