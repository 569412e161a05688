"""The checks every extension library's boundary gets, stated once over a description of the library: what its header declares,
what the shared object exports and depends on, how a refused call reports itself, and the two rules of the engine that must reach
an extension (the Mont128 latch rule, the per-thread last error).  tests/test_{mpc,prep,hm,ip,vf}_abi.py pass their own argument
builders; the red-zone tests read device_entry_points.  All five libraries come from one Makefile rule, so every check takes its
strictest form for each of them.  Every assert carries the values it compared: this is no test module, so pytest does not rewrite
them.  No torch here: the boundary is checked without a device."""
import importlib
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "secure-computation-library_amd")
OK, ERR_SIZE_MISMATCH, ERR_BAD_ARG, ERR_NO_DEVICE = 0, 1, 3, 5


@dataclass(frozen=True)
class Library:
    prefix: str              # of every symbol
    header: str              # under include/
    so: str                  # under scl_amd/
    exports: str             # the linker's version script under csrc/
    module: str              # the binding
    version_macro: str

    def path(self, what):
        return {"header": os.path.join(ROOT, "include", self.header), "so": os.path.join(PKG, "scl_amd", self.so),
                "exports": os.path.join(PKG, "csrc", self.exports)}[what]

    @property
    def lib(self):
        return importlib.import_module(self.module).lib

    def last_error(self):
        return getattr(self.lib, self.prefix + "last_error")()


def _extension(tag):
    return Library(f"scl_{tag}_", f"scl_hip_{tag}.h", f"libscl_hip_{tag}.so", f"exports_{tag}.map", f"scl_amd.{tag}", f"SCL_{tag.upper()}_ABI_VERSION")


ENGINE = Library("scl_hip_", "scl_hip.h", "libscl_hip.so", "exports.map", "scl_amd", "SCL_HIP_ABI_VERSION")
MPC, PREP, HM, IP, VF = EXTENSIONS = [_extension(tag) for tag in ("mpc", "prep", "hm", "ip", "vf")]


def header(unit):
    return open(unit.path("header")).read()


def _prototypes(unit):
    return re.sub(r"/\*.*?\*/", "", header(unit), flags=re.S)


def declared_symbols(unit):
    """every name of the library's prefix that the header declares, sorted"""
    return sorted(set(re.findall(r"\b(%s\w+)\s*\(" % unit.prefix, _prototypes(unit))))


def device_entry_points(unit):
    """the prototypes of the header that take a `_dev` pointer"""
    return sorted(m.group(1) for m in re.finditer(r"\b(%s\w+)\s*\(([^;{]*?)\)\s*;" % unit.prefix, _prototypes(unit))
                  if re.search(r"\*\s*\w+_dev\b", m.group(2)))


def expect(unit, rc, want, *words):
    """a refused call: the status, a message, and every word in it"""
    msg = unit.last_error()
    assert rc == want, (rc, want, msg)
    assert msg, f"{unit.prefix}last_error() is empty after a failure"
    for w in words:
        assert w is None or w in msg, (w, msg)


def reaches_the_device_check(unit, rc):
    """a call whose arguments are in order asks for a device next; with a GPU present these addresses must not get that far"""
    assert rc == ERR_NO_DEVICE, (rc, unit.last_error())


def check_exports(unit, symbols):
    """the header declares `symbols`, the shared object's dynamic table holds them and nothing else, and so does the version script"""
    names = declared_symbols(unit)
    assert names == symbols, (names, symbols)
    out = subprocess.run(["nm", "-D", "--defined-only", unit.path("so")], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert exported == set(names), sorted(exported ^ set(names))
    listed = re.findall(r"^\s+(%s\w+);" % unit.prefix, open(unit.path("exports")).read(), flags=re.M)
    assert sorted(listed) == names, sorted(set(listed) ^ set(names))


def check_engine_is_only_dependency(unit):
    """linked against libscl_hip.so, found beside it ($ORIGIN), and against no other extension library; every undefined scl_*
    symbol is a prototype of scl_hip.h"""
    dyn = subprocess.run(["readelf", "-d", unit.path("so")], capture_output=True, text=True, check=True).stdout
    assert "libscl_hip.so" in dyn and "$ORIGIN" in dyn, dyn
    siblings = [x.so for x in EXTENSIONS if x is not unit]
    assert len(siblings) == 4 and not any(s in dyn for s in siblings), dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", unit.path("so")], capture_output=True, text=True, check=True).stdout
    used = sorted({ln.split()[-1].split("@")[0] for ln in und.splitlines() if "scl_" in ln})
    assert used and set(used) <= set(declared_symbols(ENGINE)), used


def check_latch_rule(unit, bad_calls):
    """scl_hip_mont128_set_prime's rule reaches the extension: a worker whose latched default went stale is refused (the engine's
    own check and message) until it re-latches; the main thread, which set its own modulus, is not disturbed.  bad_calls:
    (function, arguments over Mont128, a word of its message, its status) of calls that end at a later check when the modulus is
    in order"""
    import scl_amd as scl
    p0, p1 = 2 ** 128 - 159, 2 ** 127 - 1

    def call(fn, args):
        rc = fn(*args)
        return rc, unit.last_error()
    try:
        for fn, args, word, status in bad_calls:
            assert status != OK, (word, status)
            scl.set_mont128_prime(p0)
            with ThreadPoolExecutor(max_workers=1) as worker:
                latched = worker.submit(scl.mont128_prime).result()         # the worker latches the default
                assert latched == p0, (latched, p0)
                rc, msg = worker.submit(call, fn, args).result()
                assert rc == status and word in msg, (rc, status, word, msg)
                scl.set_mont128_prime(p1)                                  # the main thread moves the default
                rc, msg = worker.submit(call, fn, args).result()
                assert rc == ERR_BAD_ARG and b"latched" in msg, (rc, msg)
                rc, msg = call(fn, args)                                   # the main thread goes on
                assert word in msg, (word, msg)
                worker.submit(scl.mont128_relatch).result()
                rc, msg = worker.submit(call, fn, args).result()
                assert rc == status and word in msg, (rc, status, word, msg)
    finally:
        scl.set_mont128_prime(p0)


def check_last_error_per_thread(unit, here, here_says, there, there_says):
    """`here` and `there` are (function, arguments) of two refused calls: the second, made on a worker thread, leaves the first
    one's message in place on this thread"""
    fn, args = here
    fn(*args)
    with ThreadPoolExecutor(max_workers=1) as worker:
        msg = worker.submit(lambda: (there[0](*there[1]), unit.last_error())).result()[1]
        assert msg.startswith(there_says), (msg, there_says)
    msg = unit.last_error()
    assert msg.startswith(here_says), (msg, here_says)
