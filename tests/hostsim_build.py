"""Builds of the TEST-ONLY host shims under tests/hostsim: one flag list for the shared libraries the
CPU tests load through ctypes, one for the stand-alone programs (the sanitizer mains, which run as
child processes: nothing is loaded into Python under a sanitizer)."""
import ctypes
import os
import shutil
import subprocess

HOSTSIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
CXX, CC = "g++", "gcc"
FLAGS = ["-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
SANITIZE = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def have_compilers():
    return shutil.which(CXX) is not None and shutil.which(CC) is not None


def source(name):
    return os.path.join(HOSTSIM, name)


def build_shim(out_dir, source, name):
    """Compile one shim into out_dir/lib<name>.so and load it."""
    so = os.path.join(str(out_dir), "lib%s.so" % name)
    subprocess.run([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", *FLAGS, "-o", so, source], check=True)
    return ctypes.CDLL(so)


def build_program(out_dir, sources, sanitize=False):
    """Compile and link the sources (C++, and C through the C compiler) into a program named after
    the first one; with sanitize under ASan + UBSan, the first report aborting.  Returns its path."""
    opt = SANITIZE if sanitize else ["-O2"]
    exe = os.path.join(str(out_dir), os.path.splitext(os.path.basename(sources[0]))[0])
    objs = []
    for src in sources:
        if src.endswith(".c"):
            obj = os.path.join(str(out_dir), os.path.basename(src) + ".o")
            subprocess.run([CC, *opt, *FLAGS, "-c", src, "-o", obj], check=True)
            objs.append(obj)
        else:
            objs.append(src)
    subprocess.run([CXX, *opt, "-std=c++17", *FLAGS, *objs, "-o", exe], check=True)
    return exe
