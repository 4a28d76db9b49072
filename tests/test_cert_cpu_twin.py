"""scripts/cert_cpu.cpp, the C++ restatement that scripts/bench_cert.py times as the CPU baseline,
against tests/certsim.py: 200 random histories, the hand cases and the five golden cases, every
status, wait, key_info and min_prepared equal.  --selfcheck walks the host arithmetic it shares with
the library (antidote_amd/csrc/am_cert_plan.h)."""
import os
import random
import subprocess

import pytest

from tests import certcases, certsim
from tests.test_abi import ROOT


@pytest.fixture(scope="module")
def cert_cpu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cert_cpu") / "cert_cpu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "antidote_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "cert_cpu.cpp"), "-o", exe], check=True)
    return exe


def run_cpu(exe, script, record=True):
    text = certcases.history_text(script, record)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    assert out.splitlines()[-1].startswith("T ")
    return certcases.parse_cpu_output(out)


def test_selfcheck_of_the_shared_host_arithmetic(cert_cpu):
    out = subprocess.run([cert_cpu, "--selfcheck"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "selfcheck ok", out.stdout + out.stderr


def test_random_histories_equal_certsim(cert_cpu):
    """200 histories in one process each would be 200 starts: they go through in 20 runs of 10, a
    new certifier (C) before each."""
    for chunk in range(20):
        text, want = "", []
        for h in range(10):
            seed = chunk * 10 + h
            rng = random.Random(1000 + seed)
            record = seed % 7 != 0
            script = certcases.random_history(rng, 30, n_keys=rng.choice([3, 16, 64]), max_tx=rng.choice([4, 24]),
                                              info_every=5, record_commits=record)
            text += certcases.history_text(script, record)
            want += certcases.expected(script, record)
        out = subprocess.run([cert_cpu], input=text, capture_output=True, text=True, check=True).stdout
        got = certcases.parse_cpu_output(out)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (chunk, i, g, w)


@pytest.mark.parametrize("case", certcases.hand_cases(), ids=[c[0] for c in certcases.hand_cases()])
def test_hand_cases_equal_certsim(cert_cpu, case):
    _, record, script = case
    assert run_cpu(cert_cpu, script, record) == certcases.expected(script, record)


@pytest.mark.parametrize("case", certcases.golden_cases(), ids=[c["name"] for c in certcases.golden_cases()])
def test_golden_cases_equal_certsim_and_the_reference(cert_cpu, case):
    script = certcases.golden_script(case)
    got = run_cpu(cert_cpu, script, case["record_commits"])
    assert got == certcases.expected(script, case["record_commits"])
    assert got[-1] is None  # nothing in flight at the end
    # and the statuses are the reference's own: replay the case through the program's answers
    answers = iter(got)
    take = lambda *_: next(answers)  # noqa: E731
    assert certsim.replay(case, take, take, take) == []


def test_values_at_the_edges_of_u64(cert_cpu):
    m = certcases.U64_MAX
    script = [("prepare", [(m, 0, m, True, [0, m]), (0, m, 0, False, [m])]), ("info", 0), ("info", m), ("min",),
              ("read", [(m, m), (m, 0), (0, m - 1), (0, m)], m), ("read", [(0, m)], 0),
              ("finish", [(m, m, True, [0, m])]), ("info", 0), ("info", m), ("min",)]
    assert run_cpu(cert_cpu, script) == certcases.expected(script)
