"""How the tests compile and run C++: the nine mirror test programs of tests/cxx/test_X_api.cc (one table, one recipe, one
staleness rule; build() compiles them through build_mirror_tests so that the binaries travel with the tree) and the stand-alone
host programs (tests/cxx/*_check.cc, compiled into a test's tmp_path, plain or under the sanitizers).  Standard library only:
build() imports this module before anything else of the tests is importable."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "tests", "cxx")
BUILD = os.path.join(CXX, "_build")
LIBDIR = os.path.join(ROOT, "secure-computation-library_amd", "scl_amd")
HIPCC = "/opt/rocm/bin/hipcc"
# address + undefined behaviour, the first report fatal; sanitizer builds are stand-alone programs with their own main
SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer")
SANITIZE_HIP_HOST = ("-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                     "-Xarch_host", "-fno-omit-frame-pointer")

# unit -> (source, the extension libraries it links in front of -lscl_hip)
MIRROR_TESTS = {
    "merkle": ("test_merkle_api.cc", ()),
    "feldman": ("test_feldman_api.cc", ()),
    "ecdsa": ("test_ecdsa_api.cc", ()),
    "pedersen": ("test_pedersen_api.cc", ()),
    "beaver": ("test_beaver_api.cc", ("scl_hip_mpc",)),
    "triples": ("test_triples_api.cc", ("scl_hip_prep", "scl_hip_mpc")),
    "hm": ("test_hm_api.cc", ("scl_hip_hm",)),
    "ip": ("test_ip_api.cc", ("scl_hip_ip", "scl_hip_hm")),
    "vf": ("test_vf_api.cc", ("scl_hip_vf",)),
}


def newest_input(source):
    """the staleness rule: the newest of include/**, the source and the test headers beside it"""
    headers = [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(ROOT, "include")) for f in fs]
    return max(os.path.getmtime(p) for p in headers + [source] + glob.glob(os.path.join(CXX, "*.hpp")))


def mirror_binary(unit, name=None, flags=("-O2",)):
    """tests/cxx/test_<unit>_api.cc compiled against the mirror and its libraries into tests/cxx/_build/<name> (build() leaves it
    in place; rebuilt here when stale) -> the path"""
    source, libs = MIRROR_TESTS[unit]
    src, exe = os.path.join(CXX, source), os.path.join(BUILD, name or source[:-len(".cc")])
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest_input(src):
        os.makedirs(BUILD, exist_ok=True)
        b = subprocess.run(["g++", "-std=c++20", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", f"-I{ROOT}/include", "-o", exe, src,
                            f"-L{LIBDIR}", *["-l" + l for l in libs], "-lscl_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-4000:]
    return exe


def build_mirror_tests():
    for unit in MIRROR_TESTS:
        mirror_binary(unit)


def needed(exe):
    """the dynamic section of a binary, for its NEEDED entries"""
    return subprocess.run(["readelf", "-d", exe], capture_output=True, text=True, check=True).stdout


def mirror_host_output(unit, name=None, flags=("-O2",)):
    """the program's --host mode: the completed process, its exit status checked"""
    r = subprocess.run([mirror_binary(unit, name, flags), "--host"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def _compile_and_run(compile_cmd, exe, args, timeout, want):
    b = subprocess.run(compile_cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and all(w in r.stdout for w in want), r.stdout + r.stderr
    return r.stdout + r.stderr


def host_check(tmp_path, source, name, flags=("-O2",), timeout=600, args=(), want=(" 0 mismatches",)):
    """a stand-alone program of tests/cxx (its own main, no library behind it) compiled by g++ into tmp_path and run: exit status
    0 and every string of `want` on its standard output -> everything it printed, on both streams"""
    exe = str(tmp_path / name)
    return _compile_and_run(["g++", "-std=c++20", *flags, f"-I{ROOT}/include", "-o", exe, os.path.join(CXX, source)], exe, args, timeout, want)


def hip_host_check(tmp_path, source, name, flags=(), timeout=120, args=(), want=(" 0 mismatches",)):
    """the same for a program that includes the kernels' headers and so goes through hipcc; it makes no HIP runtime call"""
    exe = str(tmp_path / name)
    return _compile_and_run([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", *flags, "-o", exe, os.path.join(CXX, source)], exe, args,
                            timeout, want)
