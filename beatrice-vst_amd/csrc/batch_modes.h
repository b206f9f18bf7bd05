// batch_modes.h -- the mode lattice of include/beatrice_batch.h (its "MODES" table) as code: which BeatriceBatch_* entry point is
// refused with -1 in which mode.  Plain C++17, no HIP: batch.hip gates every entry point on allowed() before it drains, binds or
// writes anything, and tests/test_cpu_mode_table.py compiles this header alone and holds it against tests/test_gpu_mode_matrix.py.
#pragma once

namespace bhip {
namespace modes {

enum class Mode { A, B, C, D, E, F, G, P, S };
constexpr int kModes = 9;

// What BeatriceBatch holds (batch.hip flags_of): the mode is derived from it here and stored nowhere.
struct Flags {
  bool tk = false, hs = false, r48 = false, rb = false, ragged = false, silent = false, pipelined = false, io = false;   // io: io_slots > 0
  int H = 1;
  bool wrap_ready = false, rates_ready = false;   // footnotes (1), (2): ConfigureWrapper / ConfigureWrapperRates has been called
};

// hs, r48 and rb imply tk and bound I/O slots, so they come before D and C; a ragged binding switches `silent` on for its own use, so
// P comes before S; `silent` beside tk is D or F with the rule enabled, and resident I/O takes stage pipelining along (C before B).
constexpr Mode mode_of(const Flags& f) {
  return f.rb ? (f.ragged ? Mode::P : Mode::G) : f.r48 ? Mode::F : f.hs ? Mode::E : f.tk ? Mode::D : f.io ? Mode::C :
         f.pipelined ? Mode::B : f.silent ? Mode::S : Mode::A;
}

// A cell is the set of conditions the call needs in that mode: none = ok, NO = refused.  H1: one hop per step; H124: one, two or four;
// WRAP / RATES: footnotes (1) / (2), once BeatriceBatch_ConfigureWrapper / ConfigureWrapperRates has been called; RULE: (3) once the
// silent-block rule is enabled in that mode; RULE_OFF: (7) while it is not.
enum Cell : unsigned { ok = 0, NO = 1, H1 = 2, H124 = 4, WRAP = 8, RATES = 16, RULE = 32, RULE_OFF = 64 };
constexpr bool holds(unsigned cell, const Flags& f) {
  return !(cell & NO) && (!(cell & H1) || f.H == 1) && (!(cell & H124) || f.H == 1 || f.H == 2 || f.H == 4) && (!(cell & WRAP) || f.wrap_ready) &&
         (!(cell & RATES) || f.rates_ready) && (!(cell & RULE) || f.silent) && (!(cell & RULE_OFF) || !f.silent);
}

// One enumerator per row of the table, in its order (StreamFrames stands for StreamFlush too; EnablePipelining is n >= 1).
enum class Entry {
  ConvertFrames, ConvertFramesDevice_ptrs, ConvertFramesDevice_NULL, ConvertBlocks48k, ConvertBlocks48kDevice_ptrs, ConvertBlocks48kDevice_NULL,
  ProcessBlocks, ProcessBlocksDevice_ptrs, ProcessBlocksDevice_NULL, FlushResidentBlocks, ProcessBlocksRagged, ProcessBlocksRaggedDevice,
  StreamFrames, EnableSilentBlockRule_1, EnableSilentBlockRule_0, SetSilentStreams, EnablePipelining, EnableTickPipeline_1, EnableTickPipeline_0,
  EnableHostStreaming_1, BindResidentIO_bind, BindResidentIO_unbind, BindResidentIO48k_bind, BindResidentBlocks_bind, BindResidentBlocksRagged_bind,
  ConfigureWrapper, ConfigureWrapperRates, ProfileKernels, TimeSteps, TimeTickLaunch, kCount
};
constexpr int kEntries = (int)Entry::kCount;

struct Row { const char* name; unsigned cell[kModes]; };
constexpr unsigned W1 = WRAP | H1, R1 = RATES | H1, W124 = WRAP | H124, T1 = H124 | RULE_OFF;
constexpr Row kTable[kEntries] = {
    // (the names are the keys of PROBES in tests/test_gpu_mode_matrix.py)   A      B      C         D         E      F     G     P     S
    {"ConvertFrames",                                                       {ok,    ok,    NO,       NO,       NO,    NO,   NO,   NO,   ok}},
    {"ConvertFramesDevice(ptrs)",                                           {ok,    ok,    NO,       NO,       NO,    NO,   NO,   NO,   ok}},
    {"ConvertFramesDevice(NULL)",                                           {ok,    ok,    ok,       ok,       NO,    NO,   NO,   NO,   ok}},
    {"ConvertBlocks48k",                                                    {H1,    NO,    NO,       NO,       NO,    NO,   NO,   NO,   H1}},
    {"ConvertBlocks48kDevice(ptrs)",                                        {H1,    NO,    NO,       NO,       NO,    NO,   NO,   NO,   H1}},
    {"ConvertBlocks48kDevice(NULL)",                                        {NO,    NO,    NO,       NO,       NO,    ok,   NO,   NO,   NO}},
    {"ProcessBlocks",                                                       {W1,    NO,    NO,       NO,       NO,    NO,   NO,   NO,   W1}},
    {"ProcessBlocksDevice(ptrs)",                                           {W1,    NO,    NO,       NO,       NO,    NO,   NO,   NO,   W1}},
    {"ProcessBlocksDevice(NULL)",                                           {NO,    NO,    NO,       NO,       NO,    NO,   ok,   NO,   NO}},
    {"FlushResidentBlocks",                                                 {NO,    NO,    NO,       NO,       NO,    NO,   ok,   ok,   NO}},
    {"ProcessBlocksRagged",                                                 {R1,    NO,    NO,       NO,       NO,    NO,   NO,   NO,   R1}},
    {"ProcessBlocksRaggedDevice",                                           {NO,    NO,    NO,       NO,       NO,    NO,   NO,   ok,   NO}},
    {"StreamFrames",                                                        {NO,    NO,    NO,       NO,       ok,    NO,   NO,   NO,   NO}},
    {"EnableSilentBlockRule(1)",                                            {H1,    NO,    RULE,     ok,       NO,    ok,   NO,   NO,   ok}},
    {"EnableSilentBlockRule(0)",                                            {ok,    ok,    ok,       ok,       ok,    ok,   NO,   NO,   ok}},
    {"SetSilentStreams",                                                    {NO,    NO,    NO,       RULE,     NO,    RULE, NO,   NO,   ok}},
    {"EnablePipelining(2)",                                                 {ok,    ok,    RULE_OFF, NO,       NO,    NO,   NO,   NO,   NO}},
    {"EnableTickPipeline(1)",                                               {NO,    NO,    T1,       RULE_OFF, NO,    NO,   NO,   NO,   NO}},
    {"EnableTickPipeline(0)",                                               {ok,    ok,    ok,       ok,       NO,    NO,   NO,   NO,   ok}},
    {"EnableHostStreaming(1)",                                              {H124,  NO,    NO,       NO,       ok,    NO,   NO,   NO,   NO}},
    {"BindResidentIO(bind)",                                                {ok,    ok,    RULE_OFF, NO,       NO,    NO,   NO,   NO,   NO}},
    {"BindResidentIO(unbind)",                                              {ok,    ok,    ok,       NO,       NO,    NO,   NO,   NO,   ok}},
    {"BindResidentIO48k(bind)",                                             {H124,  NO,    NO,       NO,       NO,    ok,   NO,   NO,   NO}},   // F, G, P: (5)
    {"BindResidentBlocks(bind)",                                            {W124,  NO,    NO,       NO,       NO,    NO,   ok,   ok,   NO}},
    {"BindResidentBlocksRagged(bind)",                                      {R1,    NO,    NO,       NO,       NO,    NO,   ok,   ok,   NO}},
    {"ConfigureWrapper",                                                    {H124,  H124,  H124,     H124,     H124,  H124, NO,   NO,   H124}},
    {"ConfigureWrapperRates",                                               {H1,    NO,    NO,       NO,       NO,    NO,   NO,   NO,   H1}},
    {"ProfileKernels",                                                      {ok,    ok,    ok,       NO,       NO,    NO,   NO,   NO,   ok}},
    {"TimeSteps",                                                           {ok,    ok,    ok,       ok,       NO,    NO,   NO,   NO,   ok}},
    {"TimeTickLaunch",                                                      {NO,    NO,    NO,       ok,       NO,    NO,   NO,   NO,   NO}},
};

constexpr bool allowed(Entry e, const Flags& f) { return holds(kTable[(int)e].cell[(int)mode_of(f)], f); }

}  // namespace modes
}  // namespace bhip
