"""A reader of include/f110_hip.h (its style is regular enough for regexes) and the comparisons of what it reads with the ctypes
mirror of red_gym_amd/_lib.py, for tests/test_abi_cpu.py.  Every comparison returns a list of differences, each a string that begins
with the symbol, struct field or constant it is about; an empty list means the two agree.
Types are strings: 'int32', 'double', ..., and with a '*' per level of pointer 'double*', 'f110_config*', 'f110_handle**'."""
import ctypes as C
import re

SCALARS = {'int': 'int32', 'int32_t': 'int32', 'int64_t': 'int64', 'uint8_t': 'uint8', 'uint32_t': 'uint32', 'uint64_t': 'uint64'}
CTYPES = {None: 'void', C.c_int32: 'int32', C.c_int64: 'int64', C.c_uint8: 'uint8', C.c_uint32: 'uint32', C.c_uint64: 'uint64',
          C.c_float: 'float', C.c_double: 'double', C.c_char_p: 'char*', C.c_void_p: '*'}     # '*': a pointer to anything
DEVICE_ONLY = ('f110_adam_state',)      # a typedef struct without a mirror: _lib holds its size alone


def _type(text):
    """'const double *a', 'f110_handle **out' or 'int32_t' as a type; the name is dropped."""
    base, stars = re.fullmatch(r'\s*(?:const\s+)?(\w+)\s*(\**)\s*\w*\s*', text).groups()
    return SCALARS.get(base, base) + stars


def _value(text, known):
    """The integer a #define's replacement text stands for: literals, defines read before and operators; else None."""
    text = re.sub(r'\b(0[xX][0-9a-fA-F]+|\d+)[uUlL]*\b', r'\1', text)
    text = re.sub(r'\bF110_\w+', lambda m: str(known.get(m.group(0), '?')), text)
    return int(eval(text, {'__builtins__': {}})) if re.fullmatch(r'[0-9a-fA-FxX()<>+\-*|&~ ]*[0-9)] *', text) else None


def read(path):
    """(defines, structs, prototypes): {name: int}, {typedef: [(field, type, array length or 0)]}, {name: (return type, [type])}."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', open(path).read(), flags=re.S)
    defines, structs, protos = {}, {}, {}
    for name, body in re.findall(r'^#define (F110_\w+)\b(.*)$', text, flags=re.M):         # the '#define F110_' lines
        if _value(body, defines) is not None:
            defines[name] = _value(body, defines)
    struct = r'typedef struct\s*\{(.*?)\}\s*(f110_\w+)\s*;'
    for body, name in re.findall(struct, text, flags=re.S):
        structs[name] = []
        for base, declarators in re.findall(r'(?:const\s+)?(\w+)\s+([^;]+);', body):       # 'const float *pre[2], *w_act[2];'
            for star, field, length in re.findall(r'(\*?)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*(?:,|$)', declarators):
                structs[name].append((field, _type(base) + star, int(defines.get(length, length or 0))))
    for ret, name, args in re.findall(r'((?:const\s+)?\w+\s*\*?)\s*\b(f110_\w+)\s*\(([^)]*)\)\s*;', re.sub(struct, ' ', text, flags=re.S)):
        assert name not in protos, name
        protos[name] = (_type(ret), [] if args.strip() in ('', 'void') else [_type(a) for a in args.split(',')])
    return defines, structs, protos


def _of_ctype(t, names):
    """A ctypes type of the table as a header type; names: mirrored class -> typedef (STRUCTS inverted)."""
    if t in CTYPES or t in names:
        return CTYPES[t] if t in CTYPES else names[t]
    return _of_ctype(t._type_, names) + '*' if issubclass(t, C._Pointer) else repr(t)


def _agree(header, table):
    return header == table or (table.startswith('*') and header.endswith(table))


def diff_prototypes(protos, symbols, restypes, structs):
    """The return type and every argument of every symbol; POINTER(S) and POINTER(scalar) of the table must meet that pointee."""
    names = {cls: name for name, cls in structs.items()}
    out = ['%s: only in the %s' % (n, 'header' if n in protos else 'table') for n in sorted(set(protos) ^ set(symbols))]
    out += ['%s: in RESTYPES but not in SYMBOLS' % n for n in sorted(set(restypes) - set(symbols))]
    for name in sorted(set(protos) & set(symbols)):
        ret, args = protos[name]
        mine = [_of_ctype(t, names) for t in symbols[name]]
        if not _agree(ret, _of_ctype(restypes.get(name, C.c_int), names)):
            out.append('%s: returns %s in the header, %s in the table' % (name, ret, _of_ctype(restypes.get(name, C.c_int), names)))
        if len(mine) != len(args):
            out.append('%s: %d arguments in the header, %d in the table' % (name, len(args), len(mine)))
        out += ['%s: argument %d is %s in the header, %s in the table' % (name, i, h, t) for i, (h, t) in enumerate(zip(args, mine)) if not _agree(h, t)]
    return out


def diff_structs(header_structs, structs):
    """Which structs are mirrored, and each one's field names, order, types (a pointer field is a c_void_p) and array lengths."""
    mirrored = {n: f for n, f in header_structs.items() if n not in DEVICE_ONLY}
    out = ['%s: only in the %s' % (n, 'header' if n in mirrored else 'table') for n in sorted(set(mirrored) ^ set(structs))]
    for name in sorted(set(mirrored) & set(structs)):
        want = [(f, '*' if t.endswith('*') else t, n) for f, t, n in mirrored[name]]
        mine = [(f, _of_ctype(getattr(t, '_length_', 0) and t._type_ or t, {}), getattr(t, '_length_', 0)) for f, t in structs[name]._fields_]
        if [w[0] for w in want] != [m[0] for m in mine]:
            out.append('%s: fields %s in the header, %s in the table' % (name, [w[0] for w in want], [m[0] for m in mine]))
        else:
            out += ['%s.%s: %s[%d] in the header, %s[%d] in the table' % ((name,) + w + m[1:]) for w, m in zip(want, mine) if w != m]
    return out


def diff_constants(defines, namespace):
    """Every F110_* integer of `namespace` (vars(_lib)) against the header's define of that name, and every E_* integer against
    F110_E_*.  F110_ADAM_STATE_BYTES is a sizeof and belongs to diff_layout."""
    mine = {'F110_' + k if k.startswith('E_') else k: v for k, v in namespace.items()
            if k.startswith(('F110_', 'E_')) and isinstance(v, int) and k != 'F110_ADAM_STATE_BYTES'}
    return ['%s: %s in the header, %d in the table' % (k, defines.get(k, 'nothing'), v) for k, v in sorted(mine.items()) if defines.get(k) != v]


def layout_program(header_structs):
    """A C program that prints 'typedef size' and 'typedef.field offset' for every struct of the header."""
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "f110_hip.h"', 'int main(void)', '{']
    for name, fields in sorted(header_structs.items()):
        lines.append('    printf("%s %%d\\n", (int)sizeof(%s));' % (name, name))
        lines += ['    printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, f, name, f) for f, _, _ in fields]
    return '\n'.join(lines + ['    return 0;', '}', ''])


def diff_layout(printed, structs, sizes):
    """What that program printed against ctypes.sizeof / .offset of `structs` and the plain byte counts of `sizes`."""
    got = {k: int(v) for k, v in (line.split() for line in printed.splitlines())}
    mine = dict(sizes, **{name: C.sizeof(cls) for name, cls in structs.items()})
    mine.update(('%s.%s' % (name, f[0]), getattr(cls, f[0]).offset) for name, cls in structs.items() for f in cls._fields_)
    return ['%s: %s by the compiler, %d in the table' % (k, got.get(k, 'nothing'), v) for k, v in sorted(mine.items()) if got.get(k) != v]
