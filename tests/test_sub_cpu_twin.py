"""scripts/sub_cpu.cpp, the C++ restatement that scripts/bench_sub.py times as the CPU baseline, against
tests/subsim.py: 200 random histories and the hand cases, every delivery, gap, counter and stream
equal.  --selfcheck walks the host arithmetic it shares with the library
(antidote_amd/csrc/am_sub_plan.h)."""
import os
import random
import subprocess

import pytest

from tests import subcases
from tests.test_abi import ROOT

CASES = subcases.hand_cases()


@pytest.fixture(scope="module")
def sub_cpu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sub_cpu") / "sub_cpu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "antidote_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "sub_cpu.cpp"), "-o", exe], check=True)
    return exe


def run_cpu(exe, script, n_dc, n_part, logging=True):
    text = subcases.history_text(script, n_dc, n_part, logging)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    assert out.splitlines()[-1].startswith("T ")
    (got,) = subcases.parse_cpu_output(out, n_part)
    return got


def test_selfcheck_of_the_shared_host_arithmetic(sub_cpu):
    out = subprocess.run([sub_cpu, "--selfcheck"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "selfcheck ok", out.stdout + out.stderr


def random_script(seed):
    rng = random.Random(5000 + seed)
    n_dc, n_part = rng.choice([1, 2, 3, 8, 32]), rng.choice([1, 2, 5])
    logging = seed % 7 != 0
    if seed % 2:
        rows, _, _ = subcases.lossy_history(rng, n_dc, n_part, 60, p_loss=0.15, p_dup=0.15, logging_enabled=logging)
    else:
        rows = subcases.random_rows(rng, n_dc, n_part, 50)
    script = subcases.split_calls(rows, [0, rng.choice([1, 3, 17])])
    if seed % 5 == 0:
        script.insert(len(script) // 3, ("set_reachable", [d for d in range(n_dc) if rng.random() < 0.5]))
        script.insert(len(script) // 2, ("set_last", rng.randrange(n_part), rng.randrange(n_dc), rng.randrange(8)))
        script.insert(2 * len(script) // 3, ("set_reachable", list(range(n_dc))))
    if seed % 11 == 0:
        script.insert(len(script) // 2, ("clear",))
    return script, n_dc, n_part, logging


def test_random_histories_equal_subsim(sub_cpu):
    """200 histories in 20 runs of 10, a new buffer (C) before each."""
    for chunk in range(20):
        text, want, dims = "", [], []
        for h in range(10):
            script, n_dc, n_part, logging = random_script(chunk * 10 + h)
            text += subcases.history_text(script, n_dc, n_part, logging)
            want.append(subcases.expected(script, n_dc, n_part, logging))
            dims.append(n_part)
        out = subprocess.run([sub_cpu], input=text, capture_output=True, text=True, check=True).stdout
        parts, cur = [], []
        for line in out.splitlines():
            cur.append(line)
            if line == "X":
                parts.append("\n".join(cur))
                cur = []
        assert len(parts) == 10
        for i, (p, w, n_part) in enumerate(zip(parts, want, dims)):
            (g,) = subcases.parse_cpu_output(p, n_part)
            assert g[0] == w[0], (chunk, i)
            assert g[1] == w[1], (chunk, i)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_cases_equal_their_literal_outputs(sub_cpu, case):
    _, n_dc, logging, steps, dropped, unexpected = case
    outs, state = run_cpu(sub_cpu, subcases.hand_script(steps), n_dc, 1, logging)
    rows = [s for s in steps if s[0] == "row"]
    assert [o[0] for o in outs] == [[s[2]] for s in rows]
    assert [o[1] for o in outs] == [[s[3]] if s[3] else [] for s in rows]
    assert sum(o[2]["dropped"] for o in outs) == dropped and sum(o[2]["unexpected"] for o in outs) == unexpected
    dc, last, mode, queue = rows[-1][4]
    assert state.get((0, dc), (0, 0, [])) == (last, mode, queue)
    assert (outs, state) == subcases.expected(subcases.hand_script(steps), n_dc, 1, logging)
    # the whole case in one call
    rest = [s for s in steps if s[0] != "row"]
    if not rest:
        (one,), state1 = run_cpu(sub_cpu, [("process", subcases.hand_rows(steps))], n_dc, 1, logging)
        assert one[0] == [sum((s[2] for s in rows), [])] and one[1] == [s[3] for s in rows if s[3]] and state1 == state


def test_an_invalid_batch_changes_nothing(sub_cpu):
    t = subcases.t
    script = [("process", [t(0, 2, 1), t(5, 6, 2)]), ("process", [t(6, 7, 3), (3, 0, 0, 0, 1, 1, {}, False, 9)]),
              ("process", [t(6, 7, 3), (0, 4, 9, 0, 1, 0, {}, False, 9)])]
    outs, state = run_cpu(sub_cpu, script, 2, 1)
    assert outs[1] == ("invalid", 8) and outs[2] == ("invalid", 7)
    assert state == {(0, 1): (2, 1, [2])}
