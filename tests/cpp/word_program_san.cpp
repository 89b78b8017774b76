// The word-program validator and host interpreter (bellman_amd/csrc/word_program.hpp) on their own, over a toy field, for a
// host sanitizer run (tests/test_word_program_cpu.py builds this file with -fsanitize=address,undefined and runs it as a
// process): a small program with every instruction kind is validated and interpreted for a few external words against
// plain integer arithmetic, then every refusal is provoked once on a copy of it, the ranges that point past their pools
// included.  Prints "word_program ok" and exits 0 when every expectation holds.
#include <stdio.h>

#include <vector>

#include "../../bellman_amd/csrc/word_program.hpp"

using namespace bh;

struct Toy {   // canonical integers below 2^61 - 1 stand for themselves
  typedef uint64_t Elem;
  static uint64_t zero() { return 0; }
  static uint64_t one() { return 1; }
  static uint64_t from_canonical(const uint64_t limbs[4]) { return (limbs[0] ^ limbs[1] ^ limbs[2] ^ limbs[3]) % 2305843009213693951ull; }
};

struct Prog {
  std::vector<WordInstr> instrs;
  std::vector<uint32_t> pool;
  std::vector<WordBit> bits;
  std::vector<WordVar> vars;
  std::vector<WordPacked> packed;
  size_t n_inputs = 2, n_aux = 0, n_ext = 2;
  WordDesc desc() const {
    return WordDesc{n_inputs, n_aux, n_ext, instrs.data(), instrs.size(), pool.data(), pool.size(), bits.data(), bits.size(),
                    vars.data(), vars.size(), packed.data(), packed.size()};
  }
};

static Prog base() {
  Prog p;
  // words: 0, 1 external; 2 CONST; 3 ROTR(0, 7); 4 SHR(1, 3); 5 XOR(3, 4); 6 AND(0, 1); 7 CH(0, 1, 2); 8 MAJ(0, 1, 2);
  // 9 ADD(0, 1, 2, 5); 10 PACK(low half of 0, high half of 1 negated)
  p.instrs = {{WORD_CONST, 0x9E3779B9u, 0, 0}, {WORD_ROTR, 0, 7, 0}, {WORD_SHR, 1, 3, 0}, {WORD_XOR, 3, 4, 0}, {WORD_AND, 0, 1, 0},
              {WORD_CH, 0, 1, 2}, {WORD_MAJ, 0, 1, 2}, {WORD_ADD, 0, 4, 0}, {WORD_PACK, 0, 0, 0}};
  p.pool = {0, 1, 2, 5};
  for (uint32_t i = 0; i < 32; i++) p.bits.push_back(i < 16 ? WordBit{0, i} : WordBit{1, i | (1u << 8)});
  for (uint32_t i = 0; i < 40; i++) p.bits.push_back(WordBit{9, i % 34});   // a packed variable of 40 bits
  p.n_aux = 36;
  for (uint32_t i = 0; i < 34; i++) p.vars.push_back(WordVar{2 + i, 9, i});   // the sum's bits, carries included
  p.vars.push_back(WordVar{36, 10, 5 | (1u << 8)});
  p.vars.push_back(WordVar{37, 8, 31});
  p.packed.push_back(WordPacked{1, 32, 40});
  return p;
}

static int expect_refusal(const Prog &p, uint32_t code, uint32_t index, int line) {
  const WordProgram w = word_program_validate(p.desc());
  if (w.status == WORD_INVALID && w.bad_code == code && w.bad_index == index) return 0;
  printf("line %d: status %d code %u index %u, wanted code %u index %u\n", line, w.status, w.bad_code, w.bad_index, code, index);
  return 1;
}
#define REFUSED(p, code, index) rc |= expect_refusal(p, code, index, __LINE__)

int main() {
  int rc = 0;
  {
    const Prog p = base();
    const WordDesc d = p.desc();
    const WordProgram w = word_program_validate(d);
    if (w.status != WORD_OK || w.n_words != 11) { printf("base refused: %u %u\n", w.bad_code, w.bad_index); return 1; }
    const uint32_t exts[4][2] = {{0, 0}, {0xFFFFFFFFu, 0xFFFFFFFFu}, {0x80000001u, 0x7FFFFFFEu}, {0x12345678u, 0x9ABCDEF0u}};
    for (const auto &e : exts) {
      std::vector<uint64_t> in(p.n_inputs), aux(p.n_aux), words(w.n_words);
      word_program_interpret(Toy(), d, w, e, in.data(), aux.data(), words.data());
      const uint32_t a = e[0], b = e[1], c = 0x9E3779B9u;
      const uint32_t x = ((a >> 7) | (a << 25)) ^ (b >> 3);
      const uint64_t sum = (uint64_t)a + b + c + x;
      const uint32_t pack = (a & 0xFFFFu) | (~b & 0xFFFF0000u);
      const uint32_t maj = (a & b) ^ (a & c) ^ (b & c);
      if (words[5] != x || words[6] != (a & b) || words[7] != ((a & b) ^ (~a & c)) || words[8] != maj || words[9] != sum || words[10] != pack) rc |= 2;
      if (in[0] != 1) rc |= 4;
      for (uint32_t i = 0; i < 34; i++)
        if (aux[i] != ((sum >> i) & 1)) rc |= 8;
      if (aux[34] != (((pack >> 5) & 1) ^ 1) || aux[35] != (maj >> 31)) rc |= 16;
      uint64_t limbs[4] = {0, 0, 0, 0};
      for (uint32_t i = 0; i < 40; i++) limbs[0] |= ((sum >> (i % 34)) & 1) << i;
      if (in[1] != Toy::from_canonical(limbs)) rc |= 32;
    }
  }
  Prog p = base(); p.instrs[3].b = 5; REFUSED(p, WORD_BAD_SOURCE, 3);                       // reads its own word
  p = base(); p.instrs[1].a = 0xFFFFFFFFu; REFUSED(p, WORD_BAD_SOURCE, 1);
  p = base(); p.pool[3] = 9; REFUSED(p, WORD_BAD_SOURCE, 7);
  p = base(); p.bits[3].word = 10; REFUSED(p, WORD_BAD_SOURCE, 8);
  p = base(); p.bits[31].bit_neg = 64; REFUSED(p, WORD_BAD_BIT, 8);
  p = base(); p.instrs[7].b = 1; REFUSED(p, WORD_BAD_ADD_ARITY, 7);
  p = base(); p.instrs[7].b = 11; REFUSED(p, WORD_BAD_ADD_ARITY, 7);
  p = base(); p.instrs[7].a = 0xFFFFFFFEu; REFUSED(p, WORD_BAD_OP, 7);                      // a range past its pool
  p = base(); p.instrs[8].a = 0xFFFFFFF0u; REFUSED(p, WORD_BAD_OP, 8);
  p = base(); p.instrs[2].b = 0; REFUSED(p, WORD_BAD_OP, 2);
  p = base(); p.instrs[0].op = 77; REFUSED(p, WORD_BAD_OP, 0);
  p = base(); p.vars[4].word = 11; REFUSED(p, WORD_BAD_VAR_SOURCE, 6);
  p = base(); p.vars[4].bit_neg = 1u << 9; REFUSED(p, WORD_BAD_VAR_SOURCE, 6);
  p = base(); p.packed[0].bits_begin = 0xFFFFFFF0u; REFUSED(p, WORD_BAD_VAR_SOURCE, 1);
  p = base(); p.packed[0].n_bits = 255; REFUSED(p, WORD_BAD_PACKED_BITS, 1);
  p = base(); p.vars[35].var = 38; REFUSED(p, WORD_BAD_VAR_RANGE, 35);
  p = base(); p.packed[0].var = 0xFFFFFFFFu; REFUSED(p, WORD_BAD_VAR_RANGE, 36);
  p = base(); p.vars.pop_back(); REFUSED(p, WORD_BAD_UNCOVERED, 37);
  p = base(); p.vars[7].var = 5; REFUSED(p, WORD_BAD_COVERED_TWICE, 5);                     // 9 lost its record, 5 has two: the lowest of them
  p = base(); p.vars[3].var = 9; REFUSED(p, WORD_BAD_UNCOVERED, 5);
  p = base(); p.vars.push_back(WordVar{0, 0, 0}); REFUSED(p, WORD_BAD_COVERED_TWICE, 0);    // ONE
  p = base(); p.vars.push_back(WordVar{1, 0, 0}); REFUSED(p, WORD_BAD_COVERED_TWICE, 1);    // packed and bit
  if (rc == 0) printf("word_program ok\n");
  return rc;
}
