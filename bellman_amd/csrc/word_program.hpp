// The word program of a gadget circuit (word_witness.hip): a straight-line program over TRACE WORDS that computes, for one
// witness, every word whose bits the circuit's variables are - what the value closures of `synthesize` compute one variable
// at a time (groth16/src/prover.rs:206) for circuits built from UInt32 gadgets.  This header is host code with no device and no
// library state, in the style of solve_plan.hpp: the validator, the ONE definition of what an instruction computes (word_exec,
// which the device kernel compiles too) and an interpreter that fills one witness on the host.  The test library reaches it
// without a context (bh_test_word_program; tests/test_word_program_cpu.py).  The field comes in through the template argument F:
//   F::Elem;  Elem zero();  Elem one();  Elem from_canonical(const uint64_t limbs[4])   (a canonical integer below the modulus)
//
// The format (the arrays of bh_word_witness_desc, include/bellman_hip.h):
//   words        a trace word is a u64.  Words 0 .. n_ext - 1 are EXTERNAL: preloaded per witness from a uint32 each.  Instruction j
//                writes word n_ext + j and reads only words below its own.
//   instructions {op, a, b, c}; the 32-bit operations read the low 32 bits of their sources and write a 32-bit value
//                CONST  a = the value            ROTR, SHR  word a by b (1 .. 31)          XOR, AND  words a, b
//                CH     (a & b) ^ (~a & c)       MAJ        (a & b) ^ (a & c) ^ (b & c)
//                ADD    the FULL sum (up to 36 bits) of the low halves of words pool[a .. a + b), 2 <= b <= 10
//                PACK   bit i of the result = bit source bits[a + i], i < 32: a word gathered from bits that are not an aligned
//                       image of one word
//   bit source   {word, bit | neg << 8}: bit `bit` (< 64) of `word`, xor neg
//   variables    (indices as bh_csr.var: 0 is ONE, inputs first, aux behind them) every variable but ONE has exactly one record:
//                bit      {var, word, bit | neg << 8}: the field element 0 or 1
//                packed   {var, bits_begin, n_bits}: sum over i < n_bits <= 254 of (bit source bits[bits_begin + i]) * 2^i
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define BH_WORD_HD __host__ __device__
#else
#define BH_WORD_HD
#endif

namespace bh {

enum : uint32_t { WORD_CONST = 1, WORD_ROTR, WORD_SHR, WORD_XOR, WORD_AND, WORD_CH, WORD_MAJ, WORD_ADD, WORD_PACK };   // BH_WORD_*
// why a program is refused (BH_WORD_BAD_*), and what the index reported with it counts
enum : uint32_t {
  WORD_BAD_SOURCE = 1,      // instruction: a source is not strictly earlier than its destination
  WORD_BAD_BIT,             // instruction (PACK): a bit index >= 64
  WORD_BAD_ADD_ARITY,       // instruction (ADD): fewer than 2 or more than 10 sources
  WORD_BAD_OP,              // instruction: unknown operation, amount outside 1 .. 31, a range outside its pool
  WORD_BAD_VAR_SOURCE,      // variable: its record names a word or a bit that does not exist
  WORD_BAD_PACKED_BITS,     // variable: packed from more than 254 bits
  WORD_BAD_VAR_RANGE,       // record (bit records first, packed behind them): its variable index is out of range
  WORD_BAD_UNCOVERED,       // variable: no record (the lowest such variable, as the solver's plan names it)
  WORD_BAD_COVERED_TWICE,   // variable: two records, or a record for ONE
};
constexpr uint32_t WORD_ADD_MIN = 2, WORD_ADD_MAX = 10, WORD_PACKED_MAX_BITS = 254, WORD_NO_INDEX = 0xFFFFFFFFu;
constexpr int WORD_OK = 0, WORD_INVALID = -2;   // BH_OK, BH_ERR_INVALID_ARG

struct WordInstr { uint32_t op, a, b, c; };               // the layout of bh_word_instr
struct WordBit { uint32_t word, bit_neg; };               // bh_word_bit
struct WordVar { uint32_t var, word, bit_neg; };          // bh_word_var
struct WordPacked { uint32_t var, bits_begin, n_bits; };  // bh_word_packed
struct WordDesc {                                         // bh_word_witness_desc
  size_t n_inputs, n_aux, n_ext;
  const WordInstr *instrs; size_t n_instrs;
  const uint32_t *pool; size_t n_pool;
  const WordBit *bits; size_t n_bits;
  const WordVar *vars; size_t n_vars;
  const WordPacked *packed; size_t n_packed;
};

// What the expansion reads per variable, 8 bytes: kind in bits 16 .. 17 of y.
//   ONE      nothing else             BIT   x = word, y & 0x1ff = bit | neg << 8          PACKED  x = bits_begin, y & 0xffff = n_bits
enum : uint32_t { WORD_REC_ONE = 0, WORD_REC_BIT = 1, WORD_REC_PACKED = 2 };
struct WordRec { uint32_t x, y; };

struct WordProgram {
  int status = WORD_OK;
  uint32_t bad_code = 0, bad_index = WORD_NO_INDEX;
  size_t n_words = 0;
  std::vector<WordRec> recs;   // per variable
};

// what one instruction computes; load(w) = trace word w of the witness at hand
template <class Load>
BH_WORD_HD inline uint64_t word_exec(const WordInstr &in, const uint32_t *pool, const WordBit *bits, Load load) {
  switch (in.op) {
    case WORD_CONST: return in.a;
    case WORD_ROTR: { const uint32_t x = (uint32_t)load(in.a); return (x >> in.b) | (x << (32 - in.b)); }
    case WORD_SHR: return (uint32_t)load(in.a) >> in.b;
    case WORD_XOR: return (uint32_t)load(in.a) ^ (uint32_t)load(in.b);
    case WORD_AND: return (uint32_t)load(in.a) & (uint32_t)load(in.b);
    case WORD_CH: { const uint32_t x = (uint32_t)load(in.a), y = (uint32_t)load(in.b), z = (uint32_t)load(in.c); return (x & y) ^ (~x & z); }
    case WORD_MAJ: { const uint32_t x = (uint32_t)load(in.a), y = (uint32_t)load(in.b), z = (uint32_t)load(in.c); return (x & y) ^ (x & z) ^ (y & z); }
    case WORD_ADD: {
      uint64_t s = 0;
      for (uint32_t i = 0; i < in.b; i++) s += (uint32_t)load(pool[in.a + i]);
      return s;
    }
    case WORD_PACK: {
      uint32_t r = 0;
      for (uint32_t i = 0; i < 32; i++) {
        const WordBit s = bits[in.a + i];
        r |= (uint32_t)(((load(s.word) >> (s.bit_neg & 63)) ^ (s.bit_neg >> 8)) & 1) << i;
      }
      return r;
    }
  }
  return 0;
}

inline WordProgram word_program_validate(const WordDesc &d) {
  WordProgram p;
  auto refuse = [&](uint32_t code, size_t index) -> WordProgram & {
    p.status = WORD_INVALID;
    p.bad_code = code;
    p.bad_index = (uint32_t)index;
    p.recs.clear();
    return p;
  };
  const size_t n_vars = d.n_inputs + d.n_aux;
  if (d.n_inputs == 0 || n_vars >= ((size_t)1 << 32) || d.n_ext + d.n_instrs >= ((size_t)1 << 32) || d.n_pool >= ((size_t)1 << 32) ||
      d.n_bits >= ((size_t)1 << 32) || (d.n_instrs && !d.instrs) || (d.n_pool && !d.pool) || (d.n_bits && !d.bits) ||
      (d.n_vars && !d.vars) || (d.n_packed && !d.packed)) {
    p.status = WORD_INVALID;   // (no code: not a fault of the program's content)
    return p;
  }
  p.n_words = d.n_ext + d.n_instrs;
  auto bit_ok = [](uint32_t bit_neg) { return (bit_neg & 0xFF) < 64 && (bit_neg >> 9) == 0; };
  for (size_t j = 0; j < d.n_instrs; j++) {
    const WordInstr &in = d.instrs[j];
    const size_t dst = d.n_ext + j;
    switch (in.op) {
      case WORD_CONST: break;
      case WORD_ROTR: case WORD_SHR:
        if (in.a >= dst) return refuse(WORD_BAD_SOURCE, j);
        if (in.b < 1 || in.b > 31) return refuse(WORD_BAD_OP, j);
        break;
      case WORD_XOR: case WORD_AND:
        if (in.a >= dst || in.b >= dst) return refuse(WORD_BAD_SOURCE, j);
        break;
      case WORD_CH: case WORD_MAJ:
        if (in.a >= dst || in.b >= dst || in.c >= dst) return refuse(WORD_BAD_SOURCE, j);
        break;
      case WORD_ADD:
        if (in.b < WORD_ADD_MIN || in.b > WORD_ADD_MAX) return refuse(WORD_BAD_ADD_ARITY, j);
        if ((size_t)in.a + in.b > d.n_pool) return refuse(WORD_BAD_OP, j);
        for (uint32_t i = 0; i < in.b; i++)
          if (d.pool[in.a + i] >= dst) return refuse(WORD_BAD_SOURCE, j);
        break;
      case WORD_PACK:
        if ((size_t)in.a + 32 > d.n_bits) return refuse(WORD_BAD_OP, j);
        for (uint32_t i = 0; i < 32; i++) {
          if ((d.bits[in.a + i].bit_neg & 0xFF) >= 64) return refuse(WORD_BAD_BIT, j);
          if (!bit_ok(d.bits[in.a + i].bit_neg)) return refuse(WORD_BAD_OP, j);
          if (d.bits[in.a + i].word >= dst) return refuse(WORD_BAD_SOURCE, j);
        }
        break;
      default: return refuse(WORD_BAD_OP, j);
    }
  }
  std::vector<uint8_t> cover(n_vars, 0);
  p.recs.assign(n_vars, WordRec{0, WORD_REC_ONE << 16});
  cover[0] = 1;   // ONE: written by the expansion itself
  auto count = [&](uint32_t v) { if (cover[v] < 2) cover[v]++; };
  for (size_t i = 0; i < d.n_vars; i++) {
    const WordVar &r = d.vars[i];
    if (r.var >= n_vars) return refuse(WORD_BAD_VAR_RANGE, i);
    if (r.word >= p.n_words || !bit_ok(r.bit_neg)) return refuse(WORD_BAD_VAR_SOURCE, r.var);
    count(r.var);
    p.recs[r.var] = WordRec{r.word, r.bit_neg | (WORD_REC_BIT << 16)};
  }
  for (size_t i = 0; i < d.n_packed; i++) {
    const WordPacked &r = d.packed[i];
    if (r.var >= n_vars) return refuse(WORD_BAD_VAR_RANGE, d.n_vars + i);
    if (r.n_bits > WORD_PACKED_MAX_BITS) return refuse(WORD_BAD_PACKED_BITS, r.var);
    if ((size_t)r.bits_begin + r.n_bits > d.n_bits) return refuse(WORD_BAD_VAR_SOURCE, r.var);
    for (uint32_t b = 0; b < r.n_bits; b++)
      if (d.bits[r.bits_begin + b].word >= p.n_words || !bit_ok(d.bits[r.bits_begin + b].bit_neg)) return refuse(WORD_BAD_VAR_SOURCE, r.var);
    count(r.var);
    p.recs[r.var] = WordRec{r.bits_begin, r.n_bits | (WORD_REC_PACKED << 16)};
  }
  for (size_t v = 0; v < n_vars; v++)
    if (cover[v] != 1) return refuse(cover[v] ? WORD_BAD_COVERED_TWICE : WORD_BAD_UNCOVERED, v);
  return p;
}

// One witness on the host from its external words (n_ext of them): inputs[n_inputs], aux[n_aux]; `words` (may be NULL)
// receives the n_words trace words.  `p` must be the validated program of `d`.
template <class F>
void word_program_interpret(const F &f, const WordDesc &d, const WordProgram &p, const uint32_t *ext, typename F::Elem *inputs,
                            typename F::Elem *aux, uint64_t *words_out) {
  std::vector<uint64_t> words(p.n_words ? p.n_words : 1);
  for (size_t e = 0; e < d.n_ext; e++) words[e] = ext[e];
  auto load = [&](uint32_t w) { return words[w]; };
  for (size_t j = 0; j < d.n_instrs; j++) words[d.n_ext + j] = word_exec(d.instrs[j], d.pool, d.bits, load);
  auto source = [&](uint32_t word, uint32_t bit_neg) { return ((words[word] >> (bit_neg & 63)) ^ (bit_neg >> 8)) & 1; };
  for (size_t v = 0; v < p.recs.size(); v++) {
    const WordRec r = p.recs[v];
    typename F::Elem &out = v < d.n_inputs ? inputs[v] : aux[v - d.n_inputs];
    const uint32_t kind = (r.y >> 16) & 3;
    if (kind == WORD_REC_ONE) {
      out = f.one();
    } else if (kind == WORD_REC_BIT) {
      out = source(r.x, r.y & 0x1FF) ? f.one() : f.zero();
    } else {
      uint64_t limbs[4] = {0, 0, 0, 0};
      for (uint32_t i = 0; i < (r.y & 0xFFFF); i++) limbs[i >> 6] |= source(d.bits[r.x + i].word, d.bits[r.x + i].bit_neg) << (i & 63);
      out = f.from_canonical(limbs);
    }
  }
  if (words_out)
    for (size_t w = 0; w < p.n_words; w++) words_out[w] = words[w];
}

}  // namespace bh
