"""Strict parser of the C subset ``include/*.h`` is written in: the one definition of the C ABI.

``parse({header name: text})`` returns what a ctypes binding needs and nothing else:

    functions  {name: (restype, [argtypes])}     every ``hrl_*`` prototype
    structs    {name: ctypes.Structure subclass}  every ``typedef struct hrl_x { ... } hrl_x;``
    constants  {name: int}                        ``#define HRL_X <integer>`` and anonymous enums' ``HRL_X = <integer>``

It never skips and never guesses: whatever is left of a header once comments, the ``#ifdef __cplusplus`` blocks,
``#include`` and the include guard are gone must be one of those three forms, or ``HeaderError`` names the header and
the declaration.  Headers may come in any order (a struct may use a constant of a header read later).
"""

import ctypes
import re

SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint8_t': ctypes.c_uint8,
           'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float, 'double': ctypes.c_double}
POINTEES = set(SCALARS) | {'void', 'char', 'int8_t'}   # what a '*' may point to, besides the headers' own structs


class HeaderError(ValueError):
    def __init__(self, header, decl, why):
        ValueError.__init__(self, '%s: %s: %r' % (header, why, ' '.join(decl.split())))


def _declare(header, where, decl, pointees, constants):
    """'const float *policy, *amask' -> [('policy', c_void_p), ('amask', c_void_p)]; the name may be absent.
    `where` is the whole declaration an error names."""
    base, _, declarators = ' '.join(re.sub(r'\bconst\b', ' ', decl).replace('*', ' * ').split()).partition(' ')
    out = []
    for d in declarators.split(','):
        m = re.fullmatch(r'\s*((?:\*\s*)*)(\w*)\s*(?:\[\s*(\w+)\s*\])?\s*', d)
        if not m:
            raise HeaderError(header, where, 'cannot type the declarator %r in' % d.strip())
        stars, name, extent = m.groups()
        if stars and base in pointees:
            ctype = ctypes.c_void_p
        elif not stars and base in SCALARS:
            ctype = SCALARS[base]
        elif base in pointees:
            raise HeaderError(header, where, '%r by value is not supported in' % base)
        else:
            raise HeaderError(header, where, 'unknown base type %r in' % base)
        if extent is not None:
            if constants is None or not (extent.isdigit() or extent in constants):
                raise HeaderError(header, where, 'an array parameter or unknown array extent %r in' % extent)
            ctype = ctype * (int(extent) if extent.isdigit() else constants[extent])
        out.append((name, ctype))
    return out


def _prototype(header, stmt, pointees):
    m = re.fullmatch(r'([\w\s*]+?)\b(hrl_[a-z0-9_]+)\s*\((.*)\)', stmt, re.S)
    if not m:
        raise HeaderError(header, stmt, 'not a prototype, a struct typedef or an anonymous enum')
    ret, name, params = ' '.join(re.findall(r'\w+|\*', m.group(1))), m.group(2), m.group(3)
    if ret != 'const char *' and ret not in SCALARS:
        raise HeaderError(header, stmt, 'unknown return type %r in' % ret)
    if '(' in params or '...' in params:
        raise HeaderError(header, stmt, 'a function pointer or a variable argument list in')
    argtypes = []
    if params.strip() != 'void':
        for p in params.split(','):
            (_, ctype), = _declare(header, stmt, p, pointees, None)   # None: no array parameters
            argtypes.append(ctype)
    return name, (ctypes.c_char_p if ret == 'const char *' else SCALARS[ret], argtypes)


def parse(headers):
    """(functions, structs, constants) of {header name: text}; see the module docstring."""
    constants, bodies, statements = {}, [], []
    for header, text in headers.items():
        text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
        text = re.sub(r'^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*', '', text,
                      flags=re.S | re.M)

        def directive(m):
            line = m.group(0)
            d = re.fullmatch(r'\s*#\s*define\s+(\w+)[ \t]*(.*)', line)
            if d and d.group(2).strip():
                v = re.fullmatch(r'\(\s*(-?\d+)\s*\)|(-?\d+)', d.group(2).strip())
                if not v:
                    raise HeaderError(header, line, '#define of something other than an integer')
                constants[d.group(1)] = int(v.group(1) or v.group(2))
            elif not d and not re.match(r'\s*#\s*(include|ifndef|endif)\b', line):
                raise HeaderError(header, line, 'unsupported preprocessor directive')
            return ''
        text = re.sub(r'^[ \t]*#[^\n]*', directive, text, flags=re.M)

        def enum(m):
            for e in filter(None, (e.strip() for e in m.group(1).split(','))):
                v = re.fullmatch(r'(HRL_\w+)\s*=\s*(-?\d+)', e)
                if not v:
                    raise HeaderError(header, e, 'enumerator without an integer value')
                constants[v.group(1)] = int(v.group(2))
            return ''
        text = re.sub(r'\benum\s*\{([^{}]*)\}\s*;', enum, text)

        def struct(m):
            if m.group(1) != m.group(3):
                raise HeaderError(header, m.group(0), 'struct tag and typedef name differ')
            bodies.append((header, m.group(1), m.group(2)))
            return ''
        text = re.sub(r'\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;', struct, text)
        statements += [(header, s.strip()) for s in text.split(';') if s.strip()]

    pointees = POINTEES | {name for _, name, _ in bodies}
    structs = {}
    for header, name, body in bodies:
        fields = [f for decl in body.split(';') if decl.strip()
                  for f in _declare(header, 'struct %s { %s; }' % (name, decl), decl, pointees, constants)]
        if not fields or not all(n for n, _ in fields):
            raise HeaderError(header, 'struct %s { %s }' % (name, body), 'no fields or a field without a name in')
        structs[name] = type(name, (ctypes.Structure,), {'_fields_': fields, '__doc__': 'struct ' + name})
    functions = {}
    for header, stmt in statements:
        name, signature = _prototype(header, stmt, pointees)
        if name in functions:
            raise HeaderError(header, stmt, 'declared twice')
        functions[name] = signature
    return functions, structs, constants
