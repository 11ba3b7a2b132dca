"""The C ABI of include/vpmi.h as ctypes objects, read from the header itself (docs/abi_binding.md).

Understands the dialect that header is written in and nothing more.  Whatever it recognises it cuts out of the text; anything but
whitespace left over, or a type outside the table below, raises AbiError naming the text -- a type is never guessed."""
import ctypes as C
import re
from types import SimpleNamespace

SCALARS = {'int': C.c_int, 'int32_t': C.c_int, 'float': C.c_float, 'size_t': C.c_size_t, 'long long': C.c_longlong}
POINTEES = {'void', 'char', 'float', 'double', 'int', 'int16_t', 'int32_t', 'int64_t', 'long long'}     # T* -> c_void_p
TYPE = r'(?:const\s+)?(long long|\w+)\s*((?:\*\s*(?:const\s*)?)*)'                            # base type, then its stars


class AbiError(ValueError):
    pass


def parse(text, class_names):
    """-> namespace(consts {name: int}, structs {C name: Structure class}, protos {name: (restype, [argtypes])})."""
    consts, structs, protos = {}, {}, {}
    scalars, pointees = dict(SCALARS), set(POINTEES)          # + the header's own void* handles and opaque structs

    def ctype(base, stars, what, ret=False):
        n = stars.count('*')
        if n == 0 and base in scalars:
            return scalars[base]
        if n == 0 and base in structs and not ret:
            return structs[base]
        if n and base in pointees:
            return C.c_char_p if ret and base == 'char' and n == 1 else C.c_void_p
        if n == 1 and base in structs:
            return C.POINTER(structs[base])
        raise AbiError(f'vpmi.h: no ctypes type for "{base}{stars.strip()}" in "{what}"')

    def bound(expr, what):                       # 7 | VP_MAX_X | VP_MAX_X - 1
        m = re.fullmatch(r'(\w+)(?:\s*-\s*(\d+))?', expr.strip())
        head = m and (int(m[1]) if m[1].isdigit() else consts.get(m[1]))
        if head is None:
            raise AbiError(f'vpmi.h: array bound "{expr}" in "{what}" is neither a literal nor a known constant')
        return head - int(m[2] or 0)

    def enum(body):
        for item in filter(None, (i.strip() for i in body.split(','))):
            m = re.fullmatch(r'(\w+)\s*=\s*(-?\d+)', item)
            if not m:
                raise AbiError(f'vpmi.h: enumerator "{item}" is not NAME = <int>')
            consts[m[1]] = int(m[2])

    def struct(body, name):
        if name not in class_names:
            raise AbiError(f'vpmi.h: struct {name} has no Python class name')
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(';'))):
            m = re.match(TYPE, decl)
            names = decl[m.end():].split(',') if m else []
            if not names or m[2] and len(names) > 1:
                raise AbiError(f'vpmi.h: cannot read the field "{decl}" of {name}')
            t = ctype(m[1], m[2], decl)
            for d in names:
                f = re.fullmatch(r'\s*(\w+)\s*(?:\[([^\]]+)\])?\s*', d)
                if not f:
                    raise AbiError(f'vpmi.h: cannot read the field "{decl}" of {name}')
                fields.append((f[1], t * bound(f[2], decl) if f[2] else t))
        structs[name] = type(class_names[name], (C.Structure,), {'_fields_': fields})

    def function(ret, stars, name, args):
        what = f'{name}({" ".join(args.split())})'
        argtypes = []
        for a in ([] if args.strip() == 'void' else args.split(',')):
            m = re.fullmatch(r'\s*' + TYPE + r'\w+\s*', a)
            if not m:
                raise AbiError(f'vpmi.h: cannot read the parameter "{a.strip()}" of {name}')
            argtypes.append(ctype(m[1], m[2], what))
        protos[name] = (None if (ret, stars) == ('void', '') else ctype(ret, stars, what, ret=True), argtypes)

    def declaration(dname, dvalue, ebody, sbody, sname, ret, stars, fname, args):
        if dname:
            consts[dname] = int(dvalue)
        elif ebody is not None:
            enum(ebody)
        elif sname:
            struct(sbody, sname)
        else:
            function(ret, stars, fname, args)
        return ''

    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#[ \t]*(ifndef \w+|ifdef \w+|define \w+|include <[\w.]+>|endif)[ \t]*$', '', text, flags=re.M)
    text = re.sub(r'\A\s*extern "C" \{(.*)\}\s*\Z', r'\1', text, flags=re.S)
    text = re.sub(r'\btypedef struct (\w+) \1;', lambda m: pointees.add(m[1]) or '', text)        # opaque: only T* appears
    text = re.sub(r'\btypedef void\s*\* (\w+);', lambda m: scalars.update({m[1]: C.c_void_p}) or '', text)
    text = re.sub(r'^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$'                       # in the header's order, so that a
                  r'|\benum \{([^{}]*)\};'                                                      # name used before its declaration
                  r'|\btypedef struct \{([^{}]*)\}\s*(\w+);'                                   # is refused, as in C
                  r'|^\s*' + TYPE + r'(\w+)\s*\(([^(){};]*)\)\s*;', lambda m: declaration(*m.groups()), text, flags=re.M)
    if text.strip():
        raise AbiError(f'vpmi.h: cannot read "{" ".join(text.split())[:120]}"')
    return SimpleNamespace(consts=consts, structs=structs, protos=protos)
