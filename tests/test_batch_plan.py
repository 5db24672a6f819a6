"""The standard loop's redo policy (BatchPlan, hyptokenizer_amd/csrc/hm_batch_plan.h) without a GPU: a
stand-alone C++ program (tests/batch_plan_driver.cpp) runs the plan against scripted outcomes, and the segments it issues
are compared with a restatement of the policy's table in Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def walk(steps, stops=(), single_found=None, sequential_stop=None):
    """The table, restated.  `stops`: (step, stop word) a pipelined segment meets, in order; single_found: what the single
    step behind a stop 6 reports when it does not merge (0 or 2); sequential_stop: step at which a sequential segment of
    more than one step finds nothing.  Returns (segments, outcomes, done, armed)."""
    stops = list(stops)
    segs, outcomes = [], []
    seg = (0, steps, True) if steps > 0 else None
    pipeline_off = single = armed = False
    done = 0
    while seg is not None:
        first, count, may = seg
        segs.append(seg)
        piped = may and count >= 2                     # (the driver's own test on the table: here always large enough)
        merged, stop = count, 0
        if piped and stops and first <= stops[0][0] < first + count:
            merged, stop = stops[0][0] - first, stops.pop(0)[1]
        elif single and single_found is not None:
            merged, stop = 0, {0: 1, 2: 2}[single_found]
        elif not piped and not single and sequential_stop is not None and first <= sequential_stop < first + count:
            merged, stop = sequential_stop - first, 1
        outcomes.append((int(piped), merged, stop))
        done, armed = first + merged, (not piped) and merged == count
        was_single, single, seg = single, False, None
        if merged == count:
            if was_single and done < steps:
                seg = (done, steps - done, not pipeline_off)
        elif piped and stop == 5:
            pipeline_off = True
            seg = (done, steps - done, False)
        elif piped and stop == 6:
            single, seg = True, (done, 1, False)
    return segs, outcomes, done, armed


CASES = (
    [dict(steps=s) for s in (0, 1, 2, 256)]
    + [dict(steps=6, stops=[(k, 5)]) for k in range(6)]
    + [dict(steps=256, stops=[(k, 6) for k in range(256)])]
    + [dict(steps=8, stops=[(3, 6)], single_found=f) for f in (0, 2)]
    + [dict(steps=8, stops=[(7, 6)]), dict(steps=8, stops=[(2, 6), (5, 5)]), dict(steps=8, stops=[(2, 6), (5, 5)], sequential_stop=6)]
    + [dict(steps=8, stops=[(4, w)]) for w in (1, 2)]
)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("batch_plan") / "batch_plan_driver")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(HERE, "batch_plan_driver.cpp"), "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)        # a compiler without the sanitizer runtimes
    return exe


def test_batch_plan_issues_the_segments_of_the_table(driver):
    script, want = [], []
    for case in CASES:
        segs, outcomes, done, armed = walk(**case)
        script += ["case %d" % case["steps"]] + ["%d %d %d" % o for o in outcomes]
        want += ["case %d" % case["steps"]] + ["seg %d %d %d" % (f, c, int(m)) for f, c, m in segs] + ["end %d %d" % (done, int(armed))]
    out = subprocess.run([driver], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout[-400:], out.stderr[-2000:])
    assert out.stdout.split("\n")[:-1] == want


def test_the_restated_table_itself():
    """What the issue of the refactor fixed in words, checked on the restatement the program is compared with."""
    assert walk(0) == ([], [], 0, False)
    assert walk(1) == ([(0, 1, True)], [(0, 1, 0)], 1, True)               # a single step is never pipelined: armed
    assert walk(256)[2:] == (256, False)                                   # one pipelined segment: not armed
    for k in range(6):                                                     # stop 5: the rest strictly sequentially
        assert walk(6, [(k, 5)]) == ([(0, 6, True), (k, 6 - k, False)], [(1, k, 5), (0, 6 - k, 0)], 6, True)
    segs, outcomes, done, armed = walk(256, [(k, 6) for k in range(256)])  # every step overflows the small tail
    assert len(segs) <= 2 * 256 + 1 and done == 256 and armed
    covered = [first + q for (first, _, _), (_, merged, _) in zip(segs, outcomes) for q in range(merged)]
    assert covered == list(range(256))                                     # [0, 256) exactly once, in order
    assert sum(1 for _, count, _ in segs if count == 1) == 256             # (the last one is the rest [255, 256) itself)
    for f in (0, 2):
        assert walk(8, [(3, 6)], single_found=f) == ([(0, 8, True), (3, 1, False)], [(1, 3, 6), (0, 0, {0: 1, 2: 2}[f])], 3, False)
    assert walk(8, [(7, 6)]) == ([(0, 8, True), (7, 1, False)], [(1, 7, 6), (0, 1, 0)], 8, True)
    assert walk(8, [(2, 6), (5, 5)])[0] == [(0, 8, True), (2, 1, False), (3, 5, True), (5, 3, False)]
    assert walk(8, [(2, 6), (5, 5)], sequential_stop=6)[2:] == (6, False)
    for w in (1, 2):
        assert walk(8, [(4, w)]) == ([(0, 8, True)], [(1, 4, w)], 4, False)
