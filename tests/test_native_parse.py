"""The strict header parser the ctypes binding is derived with (handyrl_amd/_cabi.py), on strings: no header of the
repository is read here (tests/test_abi.py pins a sample of the real ones)."""

import ctypes

import pytest

from handyrl_amd import _cabi

I, I32, I64, U64, F, D, P = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float,
                             ctypes.c_double, ctypes.c_void_p)


def functions(text):
    return _cabi.parse({'t.h': text})[0]


def test_prototype_over_several_lines():
    f = functions('''
        int hrl_scan(int alg,
                     const float *values, const float *returns,
                     int64_t B, uint64_t seed,
                     double lmb, float scale, int32_t k, uint8_t flag,
                     float *out,
                     void *stream);
    ''')
    assert f == {'hrl_scan': (I, [I, P, P, I64, U64, D, F, I32, ctypes.c_uint8, P, P])}


def test_comments_declare_nothing():
    f = functions('''
        /* hrl_ghost(int a) is gone; call hrl_scan(alg, (B, T)) instead:
         *   int hrl_ghost2(void);  */
        // int hrl_ghost3(void);
        int hrl_scan(int alg /* hrl_inner(1) */, void *stream);  /* as hrl_ghost4(x) did */
    ''')
    assert f == {'hrl_scan': (I, [I, P])}


def test_const_placement_void_and_string_return():
    f = functions('''
        int hrl_version(void);
        const char *hrl_text(int code);
        int64_t hrl_bytes(const int64_t N, int64_t const M);
        int hrl_rows(float *const *dst, const float *const *src, float const *w, const hrl_t *d, int8_t *b, int);
        typedef struct hrl_t { int64_t n; } hrl_t;
    ''')
    assert f == {'hrl_version': (I, []), 'hrl_text': (ctypes.c_char_p, [I]), 'hrl_bytes': (I64, [I64, I64]),
                 'hrl_rows': (I, [P, P, P, P, P, I])}


def test_preprocessor_frame_is_removed():
    funcs, structs, consts = _cabi.parse({'t.h': '''
        #ifndef HRL_T_H
        #define HRL_T_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        int hrl_version(void);
        #ifdef __cplusplus
        }
        #endif
        #endif /* HRL_T_H */
    '''})
    assert funcs == {'hrl_version': (I, [])} and structs == {} and consts == {}


STRUCT_H = '''
    typedef struct hrl_ring {
        int64_t N, Tm, P, A;
        int32_t nleaves;
        int32_t kind[HRL_MAX_LEAVES];
        int64_t width[HRL_MAX_LEAVES];
        const void *obs[HRL_MAX_LEAVES];
        const float *policy, *amask;
        uint8_t flags[3];
        double *const *rows;
    } hrl_ring;
'''
LIMITS_H = '#define HRL_MAX_LEAVES 8\n'


@pytest.mark.parametrize('order', [(0, 1), (1, 0)])
def test_struct_layout_with_a_constant_of_a_later_header(order):
    items = [('a_ring.h', STRUCT_H), ('b_limits.h', LIMITS_H)]
    _, structs, consts = _cabi.parse(dict(items[i] for i in order))
    ring = structs['hrl_ring']
    assert issubclass(ring, ctypes.Structure) and consts == {'HRL_MAX_LEAVES': 8}
    layout = [(n, getattr(ring, n).offset, getattr(ring, n).size) for n, _ in ring._fields_]
    # by hand: 4 x 8, 4, 8 x 4, (4 pad to 72), 8 x 8, 8 x 8, 8, 8, 3 (+5 pad), 8
    assert layout == [('N', 0, 8), ('Tm', 8, 8), ('P', 16, 8), ('A', 24, 8), ('nleaves', 32, 4), ('kind', 36, 32),
                      ('width', 72, 64), ('obs', 136, 64), ('policy', 200, 8), ('amask', 208, 8),
                      ('flags', 216, 3), ('rows', 224, 8)]
    assert ctypes.sizeof(ring) == 232
    r = ring()
    r.width[7], r.obs[7], r.policy = 5, 4096, 8192
    assert (r.width[7], r.obs[7], r.policy, r.amask) == (5, 4096, 8192, None)


def test_defines_and_anonymous_enums():
    consts = _cabi.parse({'t.h': '''
        #define HRL_OK 0
        #define HRL_EINVAL (-22)
        #define HRL_BASE ( -1000 )   /* minus a hipError_t */
        #define HRL_NEG -3
        enum {
            HRL_ALG_MC = 0,      /* first */
            HRL_ALG_TD = 1,
            HRL_ALG_LAST = -1,
        };
        enum { HRL_U8 = 0, HRL_F32 = 1 };
    '''})[2]
    assert consts == {'HRL_OK': 0, 'HRL_EINVAL': -22, 'HRL_BASE': -1000, 'HRL_NEG': -3, 'HRL_ALG_MC': 0,
                      'HRL_ALG_TD': 1, 'HRL_ALG_LAST': -1, 'HRL_U8': 0, 'HRL_F32': 1}


PAIR = 'typedef struct hrl_pair { int64_t a, b; } hrl_pair;\n'


@pytest.mark.parametrize('text,named', [
    ('int hrl_bad(size_t n);', 'hrl_bad'),                                  # unknown base type
    ('int hrl_bad(const long *p);', 'hrl_bad'),                             # unknown pointee
    ('int hrl_bad(unsigned int n);', 'hrl_bad'),
    ('void hrl_bad(int n);', 'hrl_bad'),                                    # unknown return type
    ('hrl_pair *hrl_bad(int n);\n' + PAIR, 'hrl_bad'),
    (PAIR + 'int hrl_bad(hrl_pair p);', 'hrl_bad'),                         # struct by value
    ('int hrl_bad(struct hrl_pair p);', 'hrl_bad'),
    ('int hrl_bad(union hrl_u u);', 'hrl_bad'),
    ('int hrl_bad(int8_t v);', 'hrl_bad'),                                  # a pointee-only type by value
    ('int hrl_bad(void (*done)(int), void *stream);', 'hrl_bad'),           # function pointer
    ('int hrl_bad(const char *fmt, ...);', 'hrl_bad'),                      # variable arguments
    ('int hrl_bad(int64_t shape[4]);', 'hrl_bad'),                          # array parameter
    ('int hrl_bad(int n)', 'hrl_bad'),                                      # the header ends inside a declaration
    ('int hrl_bad(int n) { return n; }', 'hrl_bad'),                        # a definition
    ('int hrl_Bad(int n);', 'hrl_Bad'),                                     # not an hrl_[a-z0-9_]+ name
    ('static inline int hrl_bad(int n);', 'hrl_bad'),
    ('int hrl_bad(int n);\nint hrl_bad(int n);', 'hrl_bad'),                # declared twice
    ('typedef int hrl_code;', 'hrl_code'),                                  # a statement of no known form
    ('extern int hrl_count;', 'hrl_count'),
    ('typedef struct hrl_s { int64_t n; void (*f)(int); } hrl_s;', '(*f)'),  # fields it cannot type
    ('typedef struct hrl_s { size_t n; } hrl_s;', 'size_t n'),
    ('typedef struct hrl_s { int64_t w[HRL_NOWHERE]; } hrl_s;', 'HRL_NOWHERE'),
    ('typedef struct hrl_s { int64_t w[2][2]; } hrl_s;', 'w[2][2]'),
    ('typedef struct hrl_s { int n : 3; } hrl_s;', 'n : 3'),
    (PAIR + 'typedef struct hrl_s { hrl_pair inner; } hrl_s;', 'hrl_pair inner'),
    ('typedef struct hrl_s { int64_t; } hrl_s;', 'int64_t'),
    ('typedef struct hrl_s { int64_t n; } hrl_t;', 'hrl_t'),
    ('#define HRL_SCALE 1.5', 'HRL_SCALE'),
    ('#define HRL_TWICE(x) (2 * (x))', 'HRL_TWICE'),
    ('#if HRL_WIDE\nint hrl_wide(void);\n#endif', 'HRL_WIDE'),              # a conditional it cannot evaluate
    ('enum { HRL_A, HRL_B };', 'HRL_A'),                                    # enumerators without values
    ('enum hrl_kind { HRL_A = 0 };', 'hrl_kind'),
])
def test_rejections_name_the_header_and_the_declaration(text, named):
    with pytest.raises(_cabi.HeaderError) as e:
        _cabi.parse({'bad.h': 'int hrl_fine(void);\n' + text + '\nint hrl_also_fine(void);'})
    assert 'bad.h' in str(e.value) and named in str(e.value)
