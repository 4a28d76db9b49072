"""scripts/dep_cpu.cpp, the C++ restatement that scripts/bench_dep.py times as the CPU baseline, against
tests/depsim.py: 200 random histories, the hand cases and u64-edge values, every delivery, clock and
queue equal.  --selfcheck walks the host arithmetic it shares with the library
(antidote_amd/csrc/am_dep_plan.h)."""
import os
import random
import subprocess

import pytest

from tests import depcases
from tests.test_abi import ROOT

CASES = depcases.hand_cases()


@pytest.fixture(scope="module")
def dep_cpu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dep_cpu") / "dep_cpu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "antidote_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "dep_cpu.cpp"), "-o", exe], check=True)
    return exe


def run_cpu(exe, script, n_dc, own, n_part, order=None):
    text = depcases.history_text(script, n_dc, own, n_part, order)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    assert out.splitlines()[-1].startswith("T ")
    (got,) = depcases.parse_cpu_output(out, n_dc, n_part)
    return got


def test_selfcheck_of_the_shared_host_arithmetic(dep_cpu):
    out = subprocess.run([dep_cpu, "--selfcheck"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "selfcheck ok", out.stdout + out.stderr


def random_script(seed):
    rng = random.Random(3000 + seed)
    n_dc, n_part = rng.choice([1, 2, 3, 8, 32]), rng.choice([1, 2, 5])
    own = rng.randrange(n_dc)
    order = None if seed % 3 else rng.sample(range(n_dc), n_dc)
    arr = depcases.random_history(rng, n_dc, n_part, 40, own, p_ping=0.1, non_monotone=seed % 4 == 0)
    script = depcases.split_calls(arr, [0, rng.choice([1, 3, 17])], 10 ** 6)
    if seed % 5 == 0:
        script.insert(len(script) // 2, ("drop_ping", True))
        script.insert(len(script) // 3, ("set_clock", rng.randrange(n_part), {rng.randrange(n_dc): rng.randint(0, 50)}))
        script.append(("drop_ping", False))
        script.append(("deliver", depcases.flush_pings(n_dc, n_part, own, 99, 10 ** 6), 10 ** 7))
    return script, n_dc, own, n_part, order


def test_random_histories_equal_depsim(dep_cpu):
    """200 histories in 20 runs of 10, a new buffer (C) before each."""
    for chunk in range(20):
        text, want, dims = "", [], []
        for h in range(10):
            script, n_dc, own, n_part, order = random_script(chunk * 10 + h)
            text += depcases.history_text(script, n_dc, own, n_part, order)
            want.append(depcases.expected(script, n_dc, own, n_part, order))
            dims.append((n_dc, n_part))
        out = subprocess.run([dep_cpu], input=text, capture_output=True, text=True, check=True).stdout
        # the histories differ in n_dc / n_part: cut the output at the X lines and parse each with its own
        parts, cur = [], []
        for line in out.splitlines():
            cur.append(line)
            if line == "X":
                parts.append("\n".join(cur))
                cur = []
        assert len(parts) == 10
        for i, (p, w, (n_dc, n_part)) in enumerate(zip(parts, want, dims)):
            (g,) = depcases.parse_cpu_output(p, n_dc, n_part)
            assert g[0] == w[0] and g[1] == w[1] and g[2] == w[2], (chunk, i)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_cases_equal_their_literal_outputs(dep_cpu, case):
    _, n_dc, own, order, steps = case
    dels, clocks, queues = run_cpu(dep_cpu, depcases.hand_script(steps), n_dc, own, 1, order)
    assert [d[0] for d in dels] == [s[2] for s in steps]
    assert clocks[0] == steps[-1][3]
    assert (dels, clocks, queues) == depcases.expected(depcases.hand_script(steps), n_dc, own, 1, order)


def test_values_at_the_edges_of_u64(dep_cpu):
    m = depcases.U64_MAX
    t = depcases.txn
    script = [("deliver", [t(1, m, {2: m, 0: m}, 1), t(2, 1, {1: m - 1}, 2), t(2, m, {}, 3, ping=True)], m),
              ("deliver", [t(1, 2 ** 63, {2: 2 ** 63}, 4), t(2, 2 ** 63, {1: 1}, 5), t(1, 1, {0: 1}, 6)], 0),
              ("set_clock", 0, {0: m, 1: 0, 2: m}), ("deliver", [t(2, 1, {1: 1}, 7)], 0)]
    assert run_cpu(dep_cpu, script, 3, 0, 1) == depcases.expected(script, 3, 0, 1)
