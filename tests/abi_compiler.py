"""What the C++ compiler says about include/vpmi.h: struct layouts and function signatures, for comparison with the ctypes binding.

The binding is read from the header (ppvector/_abi.py), so the header cannot witness it; the compiler can.  A generated C++17 file
includes vpmi.h and prints sizeof / offsetof of every struct and field and, for every function, one code per return type and
parameter taken from decltype(&vp_name) -- the type only, so nothing is linked.  A type outside the code table does not compile."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r'''
#include <cstddef>
#include <cstdio>
#include "vpmi.h"
template <class T> struct code;                       // no definition: an unexpected type is a compile error
template <> struct code<void> { static constexpr char v = 'v'; };
template <> struct code<int> { static constexpr char v = 'i'; };
template <> struct code<float> { static constexpr char v = 'f'; };
template <> struct code<long long> { static constexpr char v = 'q'; };
template <> struct code<size_t> { static constexpr char v = 'z'; };
template <class T> struct code<T*> { static constexpr char v = 'p'; };
template <class R, class... A> void sig(const char* name, R (*)(A...)) {
    const char args[] = {code<A>::v..., 0};
    std::printf("F %s %c(%s)\n", name, code<R>::v, args);
}
#define S(T) std::printf("S %s %zu\n", #T, sizeof(T));
#define M(T, f) std::printf("M %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f));
#define F(f) sig(#f, (decltype(&f))0);
int main() {
'''


def host_compiler():
    """c++, else the clang++ that hipcc drives.  The library cannot be built without one, so none is an error, not a skip."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    near = os.path.join(os.path.dirname(os.path.realpath(hipcc)), '..', 'lib', 'llvm', 'bin', 'clang++')
    for c in (shutil.which('c++'), shutil.which('clang++'), near):
        if c and os.path.exists(c):
            return c
    raise RuntimeError('no host C++ compiler (c++, clang++) found')


_seen = {}


def compiler_view(structs, functions, workdir):
    """structs {C name: [field names]}, functions [names] -> (sizes {C name: sizeof}, members {(C name, field): (offset, size)},
    signatures {name: 'r(args)'}) as the compiler sees vpmi.h.  Compiled once per process and argument set."""
    key = repr((structs, functions))
    if key not in _seen:
        body = [f'S({s})' for s in structs] + [f'M({s}, {f})' for s, fs in structs.items() for f in fs] + [f'F({f})' for f in functions]
        src, exe = os.path.join(str(workdir), 'vpmi_abi.cpp'), os.path.join(str(workdir), 'vpmi_abi')
        with open(src, 'w') as f:
            f.write(PRELUDE + '\n'.join(body) + '\nreturn 0; }\n')
        subprocess.run([host_compiler(), '-std=c++17', '-I', os.path.join(ROOT, 'include'), src, '-o', exe], check=True)
        sizes, members, sigs = {}, {}, {}
        for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
            kind, *rest = line.split()
            if kind == 'S':
                sizes[rest[0]] = int(rest[1])
            elif kind == 'M':
                members[rest[0], rest[1]] = (int(rest[2]), int(rest[3]))
            else:
                sigs[rest[0]] = rest[1]
        _seen[key] = sizes, members, sigs
    return _seen[key]


CODES = {None: 'v', C.c_int: 'i', C.c_float: 'f', C.c_longlong: 'q', C.c_size_t: 'z', C.c_void_p: 'p', C.c_char_p: 'p'}


def ctypes_view(structs, protos):
    """The same three tables from the binding: structs {C name: Structure class}, protos {name: (restype, [argtypes])}."""
    def code(t):
        return 'p' if t is not None and issubclass(t, C._Pointer) else CODES[t]
    sizes = {s: C.sizeof(cls) for s, cls in structs.items()}
    members = {(s, f): (getattr(cls, f).offset, getattr(cls, f).size) for s, cls in structs.items() for f, _ in cls._fields_}
    sigs = {name: f'{code(res)}({"".join(code(a) for a in args)})' for name, (res, args) in protos.items()}
    return sizes, members, sigs
