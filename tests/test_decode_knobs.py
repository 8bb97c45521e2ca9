"""host/decodeknobs.hpp on its own, without HIP: DecodeKnobs::fromEnv() reads the four opt-in variables of the device reading
path again at every call (a process may flip them between two batches, as these tests do with monkeypatch.setenv), each
field follows its own variable, and unset, empty, "0" and a word are off.  A stand-alone program run on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "decodeknobs.hpp"

using abub::DecodeKnobs;

static int bits(const DecodeKnobs &k) { return k.bmp | k.pngTypes << 1 | k.pngAdam7 << 2 | k.unzip << 3; }

int main()
{
    const char *const names[4] = {"ABUB_GPU_BMP", "ABUB_GPU_PNG_TYPES", "ABUB_GPU_PNG_ADAM7", "ABUB_GPU_UNZIP"};
    for (const char *n : names)
        unsetenv(n);
    assert(bits(DecodeKnobs()) == 0 && bits(DecodeKnobs::fromEnv()) == 0);
    for (int i = 0; i < 4; ++i) { // each variable alone, then off again in every way there is
        setenv(names[i], "1", 1);
        assert(bits(DecodeKnobs::fromEnv()) == 1 << i);
        for (const char *off : {"0", "", "on"}) {
            setenv(names[i], off, 1);
            assert(bits(DecodeKnobs::fromEnv()) == 0);
        }
        setenv(names[i], "2", 1);
        assert(bits(DecodeKnobs::fromEnv()) == 1 << i);
        unsetenv(names[i]);
        assert(bits(DecodeKnobs::fromEnv()) == 0);
    }
    for (int mask = 0; mask < 16; ++mask) { // every combination, each fill after a change of the environment
        for (int i = 0; i < 4; ++i)
            if (mask >> i & 1)
                setenv(names[i], "1", 1);
            else
                unsetenv(names[i]);
        assert(bits(DecodeKnobs::fromEnv()) == mask);
    }
    assert(abub::envOn("ABUB_GPU_UNZIP") && !abub::envOn("ABUB_NO_SUCH_KNOB"));
    puts("knobs OK");
    return 0;
}
"""


def test_knobs_are_read_again_at_every_fill(tmp_path):
    src, exe = str(tmp_path / "knobs.cpp"), str(tmp_path / "knobs")
    open(src, "w").write(PROGRAM)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-UNDEBUG", "-Wall", "-Wextra", "-Werror", "-I",
                         os.path.join(ROOT, "autobub3hs_amd", "host"), "-o", exe, src], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout == "knobs OK\n", (p.returncode, p.stdout, p.stderr)
