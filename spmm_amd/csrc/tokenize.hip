// Device WordPiece (spmm_wordpiece, include/spmm_hip.h): the token rows of N SMILES strings in one launch -- what tokenizer.encode_smiles
// and pad_rows make of them, one string at a time, in Python.  spmm_amd/tokenizer.py::SmilesWordPiece is normative; the table layout and the
// host form of this walk are spmm_amd/wordpiece_device.py (WordPieceTable.from_tokenizer / tokenize_host).
//
// Shape of the work: N strings of tens of bytes, each a greedy longest-match over < 256 character positions.  The longest piece matching
// AT a position does not depend on the pieces chosen before it, so one lane per position finds (len, id) on its own, and the greedy
// tokenisation is the chain p -> p + len[p] from 0.  One wave64 per string, four strings per workgroup (smiles_mask_kernel's shape).
//
// The vocabulary is a trie stored as an open-addressed HASH of (node, byte) -> child, one word per slot, plus one terminal id per node,
// staged in LDS once per workgroup.  Why a hash and not node rows: the published vocabulary makes 887 nodes over 63 distinct bytes; a
// dense node x byte-class table is 56 K entries (109 KiB at 16 bits) and would leave one workgroup per CU, while sorted child lists cost a
// search per character.  The hash at load <= 1/2 is one probe for most characters, 4 + nodes + slots words in all (2 939 words, 11.5 KiB,
// for the published vocabulary; the cap of 8 192 words = 32 KiB plus 5 KiB of strips keeps four workgroups = 16 waves on a CU).
//   table[0] = TOK_MAGIC   table[1] = nodes (node 0: root of position 0, the entries as written; node 1: root of every later position, the
//   '##' entries by their content)   table[2] = slots (a power of two)   table[3] = the longest piece in bytes
//   table[4 .. 4 + nodes)           terminal id of the node, -1: no entry ends here
//   table[4 + nodes .. + slots)     -1: empty, else (node * 128 + byte) << 12 | child; home slot (key * 0x9E3779B1) >> (32 - log2 slots),
//                                   linear probing
// A table whose header does not describe itself leaves every string to the host (status 2): nothing outside the staged words is read.
//
// Per string: the bytes (the head prepended unless the string starts with it) go to the wave's LDS strip, byte loads because string starts
// have no alignment; every lane walks the trie from its positions and parks len | id << 8; then all 64 lanes follow the chain in step (a
// broadcast read per hop, at most 256), each remembering which of ITS positions were visited, and a ballot / popcount prefix count puts the
// chosen ids into the row in order.  The chain is followed to the end of the word: an unmatched position beyond the truncation point still
// makes the row [UNK] [SEP], as in Python, which tokenises before it truncates.  Every entry of the row, lens[i] and status[i] are written
// (no pre-zeroing).  Integer state only, no atomics, plain vector stores, no inline assembly; a row's result cannot depend on the rest of
// the launch.
#include "common.h"
#include "../../include/spmm_hip.h"

namespace {

constexpr int TOK_MAGIC = 0x57500001, TOK_TABLE_MAX = 8192, TOK_NODES_MAX = 4096, TOK_PIECE_MAX = 32, TOK_CHARS_MAX = 256, TOK_HEAD_MAX = 16;

struct TokP {
  const unsigned char* blob; const long* offsets; int N, gap;
  const unsigned char* head; int head_len;
  const int* table; int table_words, max_chars, max_pieces, unk_id, sep_id, pad_id;
  int* ids; long ld; int* lens; int* status;
};

__global__ __launch_bounds__(256) void wordpiece_kernel(TokP p) {
  __shared__ int tab[TOK_TABLE_MAX];                        // the table
  __shared__ unsigned char wbytes[4][TOK_CHARS_MAX];        // the wave's word: head + string
  __shared__ int match[4][TOK_CHARS_MAX];                   // longest piece at every position: len | id << 8 (len 0: none)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int v = threadIdx.x; v < p.table_words; v += 256) tab[v] = p.table[v];
  __syncthreads();
  const int nodes = tab[1], slots = tab[2], longest = tab[3];
  const bool table_ok = tab[0] == TOK_MAGIC && nodes >= 2 && nodes <= TOK_NODES_MAX && slots >= 2 && (slots & (slots - 1)) == 0 &&
                        (long)4 + nodes + slots == (long)p.table_words && longest >= 1 && longest <= TOK_PIECE_MAX;
  const long row = (long)blockIdx.x * 4 + wave;
  const bool active = row < p.N;                            // wave-uniform; no early return: the barriers below are the workgroup's
  // ---- the word: its length, whether the head is already there, a byte outside 0x21..0x7E anywhere in it
  long beg = 0, n = 0;
  if (active) { beg = p.offsets[row]; n = p.offsets[row + 1] - p.gap - beg; }
  bool host = active && (!table_ok || n < 0);               // (offsets that run backwards: nothing of the blob is read)
  if (host) n = 0;
  bool differs = lane < p.head_len && (n < p.head_len || p.blob[beg + lane] != p.head[lane]);
  const bool has_head = __ballot(differs) == 0ull;
  const int shift = has_head ? 0 : p.head_len;
  const long wlen_l = n + shift;
  const bool fits = wlen_l <= (long)p.max_chars;            // (max_chars <= 256 was checked on the host: the strips hold the word)
  const int wlen = fits ? (int)wlen_l : 0;
  bool bad = false;
  if (active && !host) {
    if (lane < shift) {
      const unsigned char b = p.head[lane];
      bad = b < 0x21 || b > 0x7E;
      if (fits) wbytes[wave][lane] = b;
    }
    for (long j = lane; j < n; j += 64) {                   // every byte, also of a string too long to tokenise: the host decides those
      const unsigned char b = p.blob[beg + j];              // with whitespace in them, which split into shorter words
      bad |= b < 0x21 || b > 0x7E;
      if (fits) wbytes[wave][shift + (int)j] = b;
    }
  }
  host = host || __ballot(bad) != 0ull;
  const bool decide = active && !host && fits;              // wave-uniform
  __syncthreads();
  // ---- the longest piece at every position, one lane per position
  if (decide) {
    const int hshift = __clz(slots) + 1;                    // 32 - log2(slots)
    const int* term = tab + 4;
    const int* hash = tab + 4 + nodes;
    for (int q = lane; q < wlen; q += 64) {
      int node = q == 0 ? 0 : 1, best = 0, best_id = 0;
      const int stop = min(longest, wlen - q);
      for (int j = 0; j < stop; ++j) {
        const unsigned key = (unsigned)node * 128u + wbytes[wave][q + j];
        unsigned h = (key * 0x9E3779B1u) >> hshift;
        int child = -1;
        for (int probe = 0; probe < slots; ++probe) {       // (bounded: a table without an empty slot cannot hold a wave)
          const int e = hash[h];
          if (e < 0) break;
          if ((unsigned)e >> 12 == key) { child = e & 4095; break; }
          h = (h + 1) & (unsigned)(slots - 1);
        }
        if (child < 0 || child >= nodes) break;
        node = child;
        const int t = term[node];
        if (t >= 0) { best = j + 1; best_id = t; }
      }
      match[wave][q] = best | (best_id << 8);
    }
  }
  __syncthreads();
  if (!active) return;
  int* out = p.ids + row * p.ld;
  int count = 0, st = host ? 2 : 1;
  if (decide) {
    // ---- the chain from position 0, every lane the same walk; bit r of `mine`: position lane + 64 r is a piece's start
    unsigned mine = 0;
    int q = 0, pieces = 0;
    bool dead = false;
    while (q < wlen) {
      const int len = match[wave][q] & 255;
      if (len == 0) { dead = true; break; }
      if ((q & 63) == lane) mine |= 1u << (q >> 6);
      q += len;
      ++pieces;
    }
    if (!dead) {
      st = 0;
      count = min(pieces, p.max_pieces);
      int base = 0;
      for (int r = 0; r * 64 < wlen; ++r) {                 // compaction: the k-th start of the chain is entry k of the row
        const bool on = (mine >> r) & 1u;
        const unsigned long long m = __ballot(on);
        const int k = base + __popcll(m & ((1ull << lane) - 1ull));
        if (on && k < count) out[k] = match[wave][lane + 64 * r] >> 8;
        base += __popcll(m);
      }
    }
  }
  // ---- the rest of the row: [SEP] behind the pieces, then padding; [UNK] [SEP]; or nothing but padding for the host's strings
  const int len_out = st == 0 ? count + 1 : st == 1 ? 2 : 0;
  for (long j = count + lane; j < p.ld; j += 64) {
    int v = p.pad_id;
    if (st == 0 && j == count) v = p.sep_id;
    if (st == 1) v = j == 0 ? p.unk_id : j == 1 ? p.sep_id : p.pad_id;
    out[j] = v;
  }
  if (lane == 0) { p.lens[row] = len_out; p.status[row] = st; }
}

}  // namespace

extern "C" int spmm_wordpiece(const unsigned char* blob, const long* offsets, int N, int gap, const unsigned char* head, int head_len,
                              const int* table, int table_words, int max_chars, int max_pieces, int unk_id, int sep_id, int pad_id,
                              int* ids, long ld, int* lens, int* status, hipStream_t stream) {
  SPMM_CHECK_SHAPE(N >= 0, "spmm_wordpiece: N=%d (N >= 0)", N);
  SPMM_CHECK_SHAPE(gap == 0 || gap == 1, "spmm_wordpiece: gap=%d (0 or 1)", gap);
  SPMM_CHECK_SHAPE(head_len >= 0 && head_len <= TOK_HEAD_MAX, "spmm_wordpiece: head_len=%d (0 <= head_len <= 16)", head_len);
  SPMM_CHECK_SHAPE(max_chars >= 1 && max_chars <= TOK_CHARS_MAX, "spmm_wordpiece: max_chars=%d (1 <= max_chars <= 256)", max_chars);
  SPMM_CHECK_SHAPE(max_pieces >= 1, "spmm_wordpiece: max_pieces=%d (max_pieces >= 1)", max_pieces);
  SPMM_CHECK_SHAPE(ld >= (long)max_pieces + 1, "spmm_wordpiece: ld=%ld must be >= max_pieces + 1 = %ld", ld, (long)max_pieces + 1);
  SPMM_CHECK_SHAPE(table_words >= 8 && table_words <= TOK_TABLE_MAX, "spmm_wordpiece: table_words=%d (8 <= table_words <= 8192)", table_words);
  if (N == 0) return SPMM_OK;
  SPMM_CHECK_SHAPE(blob != nullptr && offsets != nullptr && table != nullptr && ids != nullptr && lens != nullptr && status != nullptr,
                   "spmm_wordpiece: blob, offsets, table, ids, lens and status are required");
  SPMM_CHECK_SHAPE(head != nullptr || head_len == 0, "spmm_wordpiece: head is required with head_len=%d", head_len);
  SPMM_CHECK_SHAPE((((uintptr_t)table | (uintptr_t)ids | (uintptr_t)lens | (uintptr_t)status) & 3) == 0,
                   "spmm_wordpiece: misaligned table / ids / lens / status (4 bytes)");
  SPMM_CHECK_SHAPE(((uintptr_t)offsets & 7) == 0, "spmm_wordpiece: misaligned offsets (8 bytes)");
  TokP p = {blob, offsets, N, gap, head, head_len, table, table_words, max_chars, max_pieces, unk_id, sep_id, pad_id, ids, ld, lens, status};
  hipLaunchKernelGGL(wordpiece_kernel, dim3((unsigned)(((long)N + 3) / 4)), dim3(256), 0, stream, p);
  SPMM_LAUNCH_CHECK("spmm_wordpiece");
  return SPMM_OK;
}
