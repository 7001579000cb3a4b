"""What the tests share around the stand-alone CPU programs of tools/ (plain module, no test; needs no GPU).

`tool` builds one of them with AddressSanitizer and UBSan, a program of its own, once per process.  The codec is the
Python half of the wire format of the model programs (tools/word_stream.h): streams of little-endian int64 words, a
float64 as its bits, a float32 as its bits in the low half of a word; `run_words` runs a program on such a stream and
`cut` makes the per-call state dicts of its output.  `layout` compiles the offsetof probe of the ABI tests."""
import functools
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(REPO, "include")
CSRC = os.path.join(REPO, "rl-environment-for-component-placement_amd", "csrc")


# ---- the builder ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tool(name, include=False, fp_contract_off=True, frame_pointer=False, more_checks=""):
    """tools/<name>.cpp as a sanitized program of its own -> its path, built once; None without g++.  The defaults are the
    line of the model programs; include: also -I include/, before csrc/; fp_contract_off=False: no -ffp-contract=off;
    frame_pointer: -fno-omit-frame-pointer; more_checks: appended to the -fsanitize= list (",float-cast-overflow")."""
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(tempfile.mkdtemp(prefix=name + "_"), name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + (["-ffp-contract=off"] if fp_contract_off else []) +
                   ["-fsanitize=address,undefined" + more_checks, "-fno-sanitize-recover=all"] + (["-fno-omit-frame-pointer"] if frame_pointer else []) +
                   (["-I", INCLUDE] if include else []) + ["-I", CSRC, "-o", exe, os.path.join(REPO, "tools", name + ".cpp")], check=True)
    return exe


# ---- the codec --------------------------------------------------------------------------------------------------------
def words(a, floats=False):
    """The int64 words of an array; floats: as float64, by their bits."""
    a = np.ascontiguousarray(a)
    return (a.astype(np.float64).view(np.int64) if floats else a.astype(np.int64)).ravel()


def float32_words(a):
    """A float32 array, each element's bits in the low half of a word."""
    return np.ascontiguousarray(a).view(np.uint32).astype(np.int64).ravel()


def bits(x):
    """The word of one float64."""
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def u64(x):
    """The word of one uint64 (given as any Python int, taken modulo 2^64)."""
    return int(np.uint64(x & (2 ** 64 - 1)).astype(np.int64))


def run_words(exe, parts):
    """Runs the program on the concatenated int64 arrays `parts` -> its output as int64 words.  Raises on a non-zero exit
    status or anything on stderr."""
    done = subprocess.run([exe], input=np.concatenate(parts).tobytes(), capture_output=True)
    assert done.returncode == 0 and done.stderr == b"", done.stderr.decode()
    return np.frombuffer(done.stdout, np.int64)


def cut(out, calls, fields, shapes, floats=(), floats32=()):
    """The output of a model program, per call the error word and then `fields` in order -> [state after call i]: dicts of
    `errors` and the fields, shaped by shapes[field] (int64; `floats` as float64, `floats32` as float32)."""
    per_call = 1 + sum(int(np.prod(shapes[f])) for f in fields)
    assert len(out) == per_call * calls
    states = []
    for i in range(calls):
        w = out[i * per_call:(i + 1) * per_call]
        st, at = {"errors": int(w[0])}, 1
        for f in fields:
            n = int(np.prod(shapes[f]))
            part = w[at:at + n]
            st[f] = (part.view(np.float64) if f in floats else part.astype(np.uint32).view(np.float32) if f in floats32 else part).reshape(shapes[f])
            at += n
        states.append(st)
    return states


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def flat(shape, *index):
    return int(np.ravel_multi_index(index, shape))


# ---- the probe --------------------------------------------------------------------------------------------------------
def layout(header, struct_name, members):
    """include/<header>'s `struct_name` as a C compiler lays it out -> ({member: offset}, sizeof), from a compiled probe."""
    tmp = tempfile.mkdtemp(prefix="layout_probe_")
    src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
    prints = "".join(f'    printf("{n} %zu\\n", offsetof({struct_name}, {n}));\n' for n in members)
    with open(src, "w") as f:
        f.write(f'#include <stddef.h>\n#include <stdio.h>\n#include "{header}"\nint main(void) {{\n'
                f'    printf("sizeof %zu\\n", sizeof({struct_name}));\n' + prints + "    return 0;\n}\n")
    subprocess.run(["g++", "-x", "c", "-std=c11", "-Wall", "-Werror", "-I", INCLUDE, "-o", exe, src], check=True)
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    size = int(got.pop("sizeof"))
    return {n: int(v) for n, v in got.items()}, size
