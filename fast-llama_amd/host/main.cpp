// main.cpp -- drop-in for the reference CLI (src/main.cpp): the same flags, the same prompt/output/summary
// lines, the per-token transformer running on an MI355X through include/flm_gpu.h.
//   ./main -c model.flm -q int8 -i "prompt" [-n 512] [-t 1.0] [-p 0.9] [-j N] [--mode gen|chat|bm] [--rounds R]
// Extra of this build: --mode score = no generation: the prompt's tokens are scored in one batched pass (flm_score_tokens) -- per position the greedy id and the probability of
// the next token, then token count, mean loss, perplexity and ms; --device <hip ordinal>; --devices a,b,... = the reference's parallel width (-j, main.cpp:30,78) on GPUs: one
// sequence sharded over the named devices (split_rows, transformer.cpp:264-287), one host thread per device; --stop-ids / --stop-seq / --stop = stop rules next to the loop's
// stop on token 0 (flm_stop_rules; one device), with a `finish_reason:` line behind the output (also printed by --mode test); --draft-model FILE = a second, small model of
// the same vocabulary drafts for the loop (flm_generate_draft; one device): the same text, several tokens per pass over the weights where the two models agree;
// --samples N = N completions of the prompt, all N drawn per pass over the weights (flm_generate_n; one device), sample j with the sampler state --seed + j;
// --prompts FILE = the file's 1 .. 16 lines as independent prompts served together, one batch per pass over the weights (flm_generate_batch; one device), prompt j with
// the sampler state --seed + j.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include <algorithm>
#include <chrono>
#include <initializer_list>
#include <iostream>
#include <string>
#include <cmath>
#include <utility>
#include <vector>

#include "engine.h"

using namespace flmhost;

namespace {
enum class Mode { GEN, CHAT, TEST, SCORE };
struct Args {
    std::string ckpt, tknr, encode_str, decode_str;
    FileType ft = FileType::UNKNOWN;
    const char* prompt = "";
    int num_threads = -1, max_tokens = 512, qtype = 2, rounds = 0, device = 0, seed = 128391297;
    float topp = 0.9f, temp = 1.0f;
    bool use_numa = false, detail = false, debug = false;
    std::vector<int> devices;
    const char* bad_devices = nullptr;      // a --devices argument that did not parse
    int samples = 0; const char* bad_samples = nullptr;      // --samples N: 1..16 completions of the prompt (0 = off)
    const char* prompts_file = nullptr; std::vector<std::string> prompts;      // --prompts FILE: one prompt per line, 1..16 lines
    int batch_rows = -1; const char* bad_batch_rows = nullptr;      // --batch-rows N (with --prompts): the prompts enter inside the steps' passes, at most N prompt rows per pass (0: no bound; -1 = off)
    int lookup_k = 0, lookup_g = 3;         // --lookup K[,G]: draft length (4..15; 0 = off) and longest n-gram (1..8) of the prompt-lookup drafter
    const char* bad_lookup = nullptr;
    int draft_k = 0, draft_g = 3;           // --draft K[,G]: the same drafter and ranges at whatever temperature the run has (-t 0: flm_generate_lookup, else flm_generate_lookup_sample)
    const char* bad_draft = nullptr;
    std::string draft_model;                // --draft-model FILE: a small model of the same vocabulary drafts instead of the prompt lookup (flm_generate_draft; K of --draft, 7 without it)
    // the sampling controls (flm_sampling): any of these flags switches the shaping stage on
    bool shape_set = false; ShapeControls shape; int repeat_last_n = 64;
    std::vector<int32_t> bias_ids; std::vector<float> bias_values; const char* bad_sampling = nullptr;
    // --typical P / --mirostat 2 [--mirostat-ent TAU] [--mirostat-lr ETA]: the entropy-driven samplers (flm_entropy); mu starts at 2 TAU
    bool ent_set = false; float typical = 0.0f; int mirostat = 0; float miro_tau = 5.0f, miro_eta = 0.1f;
    int logprobs_n = -1; bool logprobs_shaped = false; const char* bad_logprobs = nullptr;   // --logprobs N[,shaped]: top-N alternatives per generated token (0..20; -1 = off), from the raw or the shaped row
    // --stop-ids a,b,... / --stop-seq a,b,... (repeatable) / --stop STR (repeatable): stop rules next to the loop's own stop on token 0
    std::vector<int32_t> stop_ids; std::vector<std::vector<int32_t>> stop_seqs; std::vector<std::string> stop_strs; const char* bad_stop = nullptr;
    const char* constraint = nullptr;       // --constraint FILE: a token-level DFA in the `flm-dfa 1 <n_states>` text format
    std::vector<int32_t> dfa_row, dfa_tok, dfa_nxt;
    Mode mode = Mode::GEN;
    bool mode_test = false;                 // --mode test: the benchmark mode under the spelling that also prints the finish reason (benchmark / bm print what they always did)
};
const char* Y = "\x1b[33m"; const char* G = "\x1b[32m"; const char* E = "\x1b[0m";

void usage(const char* bin) {
    fprintf(stderr, "Usage:\n   %s [OPTIONS]\nOptions:\n", bin);
    fprintf(stderr, "   --checkpoint,-c   <string>    the file path of the model checkpoint\n");
    fprintf(stderr, "   --tokenizer,-z    <string>    the file path of the tokenizer\n");
    fprintf(stderr, "   --file-type,-f    <string>    flm | gguf | llama2c\n");
    fprintf(stderr, "   --mode            <string>    gen | chat | benchmark(bm) | score (this build only: per-token probabilities and the perplexity of the prompt) | test (this build only: benchmark, with a `finish_reason:<why>\\trule:<n>` line per round)\n");
    fprintf(stderr, "   --prompt,-i       <string>    the input prompt text\n");
    fprintf(stderr, "   --max-tokens,-n   <integer>   the maximum number of generated tokens\n");
    fprintf(stderr, "   --temperature,-t  <float>     the value for temperature sampling, [0, 1]\n");
    fprintf(stderr, "   --topp,-p         <float>     the value for top-p sampling, [0, 1]\n");
    fprintf(stderr, "   --quant,-q        <string>    quantization type, can be INT8, INT16\n");
    fprintf(stderr, "   --threads,-j      <number>    accepted for compatibility (the GPU build has no worker threads)\n");
    fprintf(stderr, "   --device          <number>    HIP device ordinal (this build only)\n");
    fprintf(stderr, "   --devices         <a,b,...>   shard ONE sequence over these HIP devices, 1 to 8 of them (this build only)\n");
    fprintf(stderr, "   --lookup          <K[,G]>     with -t 0 on one device: draft K (4..15) tokens per step by prompt lookup (n-grams up to G, 1..8, default 3) and verify them in one pass; the same text (this build only)\n");
    fprintf(stderr, "   --draft           <K[,G]>     on one device, at any temperature: draft K (4..15) tokens per step by prompt lookup (n-grams up to G, 1..8, default 3) and verify them in one pass, sampled rows drawn with the sampler's own coins; the same text (this build only)\n");
    fprintf(stderr, "   --draft-model     <file>      on one device, at any temperature: a second, small model of the same vocabulary (quantisation: the file's own or -q) drafts the K tokens of --draft (default 7) instead of the prompt lookup; the same text (this build only)\n");
    fprintf(stderr, "   --prompts         <FILE>      on one device: the file's lines (1..16, one prompt per line) as independent prompts served together, one batch per pass over the weights, the completions printed in the file's order, each behind a line `--- prompt j ---`; prompt j's sampler state is --seed + j; not with --samples or the other extras of this build (this build only)\n");
    fprintf(stderr, "   --batch-rows      <N>         with --prompts: the prompts enter inside the steps' passes over the weights, at most N prompt rows per pass (0: no bound), instead of one pass per prompt; the same completions (this build only)\n");
    fprintf(stderr, "   --samples         <N>         on one device: N (1..16) completions of the prompt, all N drawn per pass over the weights, printed one after another, each behind a line `--- sample j ---`; sample j's sampler state is --seed + j (here --seed counts); not with the other extras of this build (this build only)\n");
    fprintf(stderr, "   --top-k           <integer>   keep the K most likely tokens, 0 = off (this build only)\n");
    fprintf(stderr, "   --min-p           <float>     drop tokens whose probability is below this fraction of the most likely one's, [0, 1), 0 = off (this build only)\n");
    fprintf(stderr, "   --repeat-penalty  <float>     penalise the tokens of the last --repeat-last-n ids, > 0, 1 = off (this build only)\n");
    fprintf(stderr, "   --repeat-last-n   <integer>   the penalties' window, 0 .. 1024, default 64 (this build only)\n");
    fprintf(stderr, "   --presence-penalty  <float>   subtracted once from every token of the window, 0 = off (this build only)\n");
    fprintf(stderr, "   --frequency-penalty <float>   subtracted per occurrence in the window, 0 = off (this build only)\n");
    fprintf(stderr, "   --logit-bias      <id=val[,id=val...]>  added to these tokens' logits; -inf bans a token; at most 256 pairs (this build only)\n");
    fprintf(stderr, "   --typical         <float>     locally typical sampling: keep the tokens whose surprise is closest to the distribution's entropy, up to this probability mass, (0, 1), 1 = off (this build only)\n");
    fprintf(stderr, "   --mirostat        <0|2>       2: Mirostat v2 -- keep the tokens whose surprise (bits) is at most a running state that follows --mirostat-ent; top-p is ignored; 0 = off (this build only)\n");
    fprintf(stderr, "   --mirostat-ent    <float>     Mirostat's target entropy tau, default 5; the state starts at 2 tau (this build only)\n");
    fprintf(stderr, "   --mirostat-lr     <float>     Mirostat's learning rate eta, default 0.1 (this build only)\n");
    fprintf(stderr, "   --constraint      <file>      mask every generated token with a token-level DFA, armed at state 0: a `flm-dfa 1 <n_states>` line, then `state token next` per line (this build only)\n");
    fprintf(stderr, "   --logprobs        <N[,shaped]>  on one device: after the text, one line per generated token `index id logprob | id:logprob ...` with the N (0..20) most likely alternatives, from the model's own distribution or (shaped) the row the sampler read (this build only)\n");
    fprintf(stderr, "   --stop-ids        <a,b,...>   on one device: end the output at the first of these token ids too (delivered, like token 0), at most 64 distinct ids (this build only)\n");
    fprintf(stderr, "   --stop-seq        <a,b,...>   on one device: end the output behind this sequence of 1..32 token ids; repeatable, at most 16 sequences with --stop (this build only)\n");
    fprintf(stderr, "   --stop            <string>    the same for a string, tokenised once without BOS: a token-level match on that one tokenisation; repeatable; a string of more than 32 tokens is reported once the model (its tokenizer) is loaded (this build only)\n");
    fprintf(stderr, "                                 with any of the three a line `finish_reason:<length|stop_token|stop_id|stop_seq|cancel>\\trule:<n>` follows the output\n");
    fprintf(stderr, "   --encode,-e       <string>    encode the input string into tokens\n");
    fprintf(stderr, "   --decode,-d       <string>    decode the input tokens to text\n");
    fprintf(stderr, "   --help,-h                     print this message\n");
}

// The flag set is the drop-in surface (the reference's Arguments::parse, main.cpp:171-244, accepts the same spellings); here it is a table: one row per flag with what it
// stores, so that the two builds' flags can be compared row by row and a new flag is one line.
namespace {
bool parse_devices(const char* v, std::vector<int>& out) {      // a comma-separated list of 1 to 8 non-negative ordinals, nothing else
    out.clear();
    bool ok = *v != 0;
    while (ok && *v) {
        char* e; const long d = strtol(v, &e, 10);
        ok = e != v && d >= 0 && d < 1024 && (*e == 0 || (*e == ',' && e[1] != 0)) && out.size() < 8;
        if (ok) { out.push_back((int)d); v = *e ? e + 1 : e; }
    }
    return ok;
}
bool parse_draft(const char* v, int& k_out, int& g_out) {       // K or K,G with 4 <= K <= 15 and 1 <= G <= 8 (default 3), nothing else
    char* e; const long k = strtol(v, &e, 10); long g = 3;
    bool ok = e != v && k >= 4 && k <= 15;
    if (ok && *e == ',') { const char* s = e + 1; g = strtol(s, &e, 10); ok = e != s && g >= 1 && g <= 8; }
    if (!ok || *e != 0) return false;
    k_out = (int)k; g_out = (int)g;
    return true;
}
bool parse_logprobs(const char* v, int& n_out, bool& shaped_out) {   // N or N,shaped with 0 <= N <= 20, nothing else
    char* e; const long n = strtol(v, &e, 10);
    if (e == v || n < 0 || n > FLM_LOGPROBS_MAX || (*e != 0 && strcmp(e, ",shaped") != 0)) return false;
    n_out = (int)n; shaped_out = *e != 0;
    return true;
}
bool parse_ids(const char* v, size_t max_n, std::vector<int32_t>& out) {      // a comma-separated list of 1 to max_n non-negative ids, nothing else
    out.clear();
    bool ok = *v != 0;
    while (ok && *v) {
        char* e; const long d = strtol(v, &e, 10);
        ok = e != v && *v >= '0' && *v <= '9' && d >= 0 && d <= 0x7ffffffe && (*e == 0 || (*e == ',' && e[1] != 0)) && out.size() < max_n;
        if (ok) { out.push_back((int32_t)d); v = *e ? e + 1 : e; }
    }
    return ok;
}
bool parse_float(const char* v, float& out) { char* e; const float f = strtof(v, &e); if (e == v || *e != 0) return false; out = f; return true; }
bool parse_bias(const char* v, std::vector<int32_t>& ids, std::vector<float>& vals) {       // id=val[,id=val...], val a float or -inf, at most 256 pairs
    ids.clear(); vals.clear();
    bool ok = *v != 0;
    while (ok && *v) {
        char* e; const long id = strtol(v, &e, 10);
        ok = e != v && id >= 0 && *e == '=' && ids.size() < 256;
        if (!ok) break;
        const char* s = e + 1; const float b = strtof(s, &e);
        ok = e != s && (*e == 0 || (*e == ',' && e[1] != 0)) && b == b && b != INFINITY;
        if (ok) { ids.push_back((int32_t)id); vals.push_back(b); v = *e ? e + 1 : e; }
    }
    return ok;
}
template <class E> bool pick(const char* v, std::initializer_list<std::pair<const char*, E>> names, E& out) {     // case-insensitive keyword -> enum; unknown words leave `out` alone (as the reference does)
    for (const auto& n : names) if (!strcasecmp(v, n.first)) { out = n.second; return true; }
    return false;
}
struct Flag {
    const char* short_name; const char* long_name; bool takes_value;
    void (*apply)(Args& a, const char* v);
};
const Flag kFlags[] = {
    {"-j", "--threads",        true,  [](Args& a, const char* v) { a.num_threads = atoi(v); }},
    {"-q", "--quant",          true,  [](Args& a, const char* v) { pick<int>(v, {{"int16", 1}, {"int8", 2}, {"int4", 3}}, a.qtype); }},
    {nullptr, "--numa",        false, [](Args& a, const char*) { a.use_numa = true; }},
    {nullptr, "--uma",         false, [](Args& a, const char*) { a.use_numa = false; }},
    {nullptr, "--detail",      false, [](Args& a, const char*) { a.detail = true; }},
    {nullptr, "--debug",       false, [](Args& a, const char*) { a.debug = true; a.detail = true; }},
    {"-c", "--checkpoint",     true,  [](Args& a, const char* v) { a.ckpt = v; }},
    {"-z", "--tokenizer",      true,  [](Args& a, const char* v) { a.tknr = v; }},
    {"-f", "--file-type",      true,  [](Args& a, const char* v) { pick<FileType>(v, {{"flm", FileType::FLM}, {"gguf", FileType::GGUF}, {"llama2c", FileType::LLAMA2C}}, a.ft); }},
    {"-i", "--prompt",         true,  [](Args& a, const char* v) { a.prompt = v; }},
    {"-e", "--encode",         true,  [](Args& a, const char* v) { a.encode_str = v; }},
    {"-d", "--decode",         true,  [](Args& a, const char* v) { a.decode_str = v; }},
    {"-n", "--max-new-tokens", true,  [](Args& a, const char* v) { a.max_tokens = atoi(v); }},
    {"-p", "--topp",           true,  [](Args& a, const char* v) { a.topp = (float)atof(v); }},
    {"-t", "--temperature",    true,  [](Args& a, const char* v) { a.temp = (float)atof(v); }},
    {nullptr, "--seed",        true,  [](Args& a, const char* v) { a.seed = atoi(v); }},
    {nullptr, "--rounds",      true,  [](Args& a, const char* v) { a.rounds = atoi(v); }},
    {"-m", "--mode",           true,  [](Args& a, const char* v) { pick<Mode>(v, {{"gen", Mode::GEN}, {"generate", Mode::GEN}, {"chat", Mode::CHAT}, {"benchmark", Mode::TEST}, {"bm", Mode::TEST}, {"test", Mode::TEST}, {"score", Mode::SCORE}}, a.mode); a.mode_test = !strcasecmp(v, "test"); }},
    {nullptr, "--device",      true,  [](Args& a, const char* v) { a.device = atoi(v); }},                                  // (this build only)
    {nullptr, "--devices",     true,  [](Args& a, const char* v) { if (!parse_devices(v, a.devices)) a.bad_devices = v; }},   // (this build only)
    {nullptr, "--lookup",      true,  [](Args& a, const char* v) {                                                            // (this build only)
        char* e; const long k = strtol(v, &e, 10); long g = 3;
        bool ok = e != v && k >= 4 && k <= 15;
        if (ok && *e == ',') { const char* s = e + 1; g = strtol(s, &e, 10); ok = e != s && g >= 1 && g <= 8; }
        if (ok && *e == 0) { a.lookup_k = (int)k; a.lookup_g = (int)g; } else a.bad_lookup = v; }},
    {nullptr, "--draft",       true,  [](Args& a, const char* v) { if (!parse_draft(v, a.draft_k, a.draft_g)) a.bad_draft = v; }},                 // (this build only)
    {nullptr, "--prompts",     true,  [](Args& a, const char* v) { a.prompts_file = v; }},   // (this build only)
    {nullptr, "--batch-rows",  true,  [](Args& a, const char* v) { char* e; const long k = strtol(v, &e, 10); if (e == v || *e || k < 0 || k > 1000000) a.bad_batch_rows = v; else a.batch_rows = (int)k; }},   // (this build only)
    {nullptr, "--samples",     true,  [](Args& a, const char* v) { char* e; const long k = strtol(v, &e, 10); if (e == v || *e || k < 1 || k > FLM_FAN_MAX) a.bad_samples = v; else a.samples = (int)k; }},   // (this build only)
    {nullptr, "--draft-model", true,  [](Args& a, const char* v) { a.draft_model = v; }},                                                                                          // (this build only)
    {nullptr, "--top-k",             true, [](Args& a, const char* v) { char* e; const long k = strtol(v, &e, 10); a.shape_set = true; if (e == v || *e || k < 0 || k > 0x7fffffff) a.bad_sampling = v; else a.shape.top_k = (int)k; }},   // (this build only)
    {nullptr, "--min-p",             true, [](Args& a, const char* v) { a.shape_set = true; if (!parse_float(v, a.shape.min_p) || !(a.shape.min_p >= 0.f && a.shape.min_p < 1.f)) a.bad_sampling = v; }},                              // (this build only)
    {nullptr, "--repeat-penalty",    true, [](Args& a, const char* v) { a.shape_set = true; if (!parse_float(v, a.shape.repeat_penalty) || !(a.shape.repeat_penalty > 0.f) || a.shape.repeat_penalty == INFINITY) a.bad_sampling = v; }},   // (this build only)
    {nullptr, "--repeat-last-n",     true, [](Args& a, const char* v) { char* e; const long k = strtol(v, &e, 10); a.shape_set = true; if (e == v || *e || k < 0 || k > 1024) a.bad_sampling = v; else a.repeat_last_n = (int)k; }},         // (this build only)
    {nullptr, "--presence-penalty",  true, [](Args& a, const char* v) { a.shape_set = true; if (!parse_float(v, a.shape.presence_penalty) || a.shape.presence_penalty != a.shape.presence_penalty) a.bad_sampling = v; }},               // (this build only)
    {nullptr, "--frequency-penalty", true, [](Args& a, const char* v) { a.shape_set = true; if (!parse_float(v, a.shape.frequency_penalty) || a.shape.frequency_penalty != a.shape.frequency_penalty) a.bad_sampling = v; }},            // (this build only)
    {nullptr, "--typical",           true, [](Args& a, const char* v) { a.ent_set = true; if (!parse_float(v, a.typical) || a.typical != a.typical) a.bad_sampling = v; }},                                                          // (this build only)
    {nullptr, "--mirostat",          true, [](Args& a, const char* v) { char* e; const long k = strtol(v, &e, 10); a.ent_set = true; if (e == v || *e || (k != 0 && k != 2)) a.bad_sampling = v; else a.mirostat = (int)k; }},          // (this build only)
    {nullptr, "--mirostat-ent",      true, [](Args& a, const char* v) { a.ent_set = true; if (!parse_float(v, a.miro_tau) || !std::isfinite(a.miro_tau)) a.bad_sampling = v; }},                                                     // (this build only)
    {nullptr, "--mirostat-lr",       true, [](Args& a, const char* v) { a.ent_set = true; if (!parse_float(v, a.miro_eta) || !std::isfinite(a.miro_eta)) a.bad_sampling = v; }},                                                     // (this build only)
    {nullptr, "--logprobs",          true, [](Args& a, const char* v) { if (!parse_logprobs(v, a.logprobs_n, a.logprobs_shaped)) a.bad_logprobs = v; }},                                                                          // (this build only)
    {nullptr, "--stop-ids",          true, [](Args& a, const char* v) {                                                                                                                                                             // (this build only)
        std::vector<int32_t> ids; bool ok = parse_ids(v, FLM_STOP_IDS_MAX, ids);
        for (size_t i = 0; ok && i < ids.size(); ++i) for (size_t k = 0; k < i; ++k) ok = ok && ids[k] != ids[i];
        for (size_t i = 0; ok && i < ids.size(); ++i) ok = std::find(a.stop_ids.begin(), a.stop_ids.end(), ids[i]) == a.stop_ids.end();
        if (ok && a.stop_ids.size() + ids.size() <= (size_t)FLM_STOP_IDS_MAX) a.stop_ids.insert(a.stop_ids.end(), ids.begin(), ids.end()); else a.bad_stop = v; }},
    {nullptr, "--stop-seq",          true, [](Args& a, const char* v) { std::vector<int32_t> q; if (parse_ids(v, FLM_STOP_SEQ_LEN_MAX, q)) a.stop_seqs.push_back(q); else a.bad_stop = v; }},                                       // (this build only)
    {nullptr, "--stop",              true, [](Args& a, const char* v) { if (*v) a.stop_strs.push_back(v); else a.bad_stop = "--stop with an empty string"; }},                                                                    // (this build only)
    {nullptr, "--constraint",        true, [](Args& a, const char* v) { a.constraint = v; }},                                                                                                                                      // (this build only)
    {nullptr, "--logit-bias",        true, [](Args& a, const char* v) { a.shape_set = true; if (!parse_bias(v, a.bias_ids, a.bias_values)) a.bad_sampling = v; }},                                                                      // (this build only)
};
}
void parse(Args& a, int argc, const char** argv) {
    for (int i = 1; i < argc;) {
        const std::string arg = argv[i++];
        if (arg == "-h" || arg == "--help") { usage(argv[0]); exit(0); }
        const Flag* hit = nullptr;
        for (const Flag& f : kFlags) if ((f.short_name && arg == f.short_name) || arg == f.long_name) { hit = &f; break; }
        if (!hit) { fprintf(stderr, "Unknown argument:\x1b[31m%s\x1b[0m\n", arg.c_str()); usage(argv[0]); exit(-1); }
        const char* v = nullptr;
        if (hit->takes_value) { if (i >= argc) { usage(argv[0]); exit(-1); } v = argv[i++]; }
        hit->apply(a, v);
        if (a.bad_devices) { fprintf(stderr, "Invalid --devices list:\x1b[31m%s\x1b[0m (expected 1 to 8 HIP device ordinals, e.g. 0,1,2,3)\n", a.bad_devices); usage(argv[0]); exit(-1); }
    }
    if (a.bad_lookup) { fprintf(stderr, "Invalid --lookup:\x1b[31m%s\x1b[0m (expected K or K,G with 4 <= K <= 15 and 1 <= G <= 8)\n", a.bad_lookup); usage(argv[0]); exit(-1); }
    if (a.prompts_file) {      // a file that cannot be read, or whose line count is out of range, is a usage error, before any model is loaded
        FILE* f = fopen(a.prompts_file, "rb");
        std::string line; int ch; bool any = false;
        while (f && (ch = fgetc(f)) != EOF) {
            if (ch == '\n') { a.prompts.push_back(line); line.clear(); any = false; }
            else { line.push_back((char)ch); any = true; }
        }
        if (f) fclose(f);
        if (any) a.prompts.push_back(line);
        for (auto& p : a.prompts) if (!p.empty() && p.back() == '\r') p.pop_back();
        bool empty_line = false; for (const auto& p : a.prompts) empty_line = empty_line || p.empty();
        if (!f || a.prompts.empty() || a.prompts.size() > FLM_BATCH_MAX || empty_line) {
            fprintf(stderr, "Invalid --prompts file:\x1b[31m%s\x1b[0m (expected a readable file of 1 to 16 non-empty lines, one prompt per line)\n", a.prompts_file); usage(argv[0]); exit(-1);
        }
    }
    if (a.bad_batch_rows) { fprintf(stderr, "Invalid --batch-rows:\x1b[31m%s\x1b[0m (expected a number of prompt rows per pass, 0 for no bound)\n", a.bad_batch_rows); usage(argv[0]); exit(-1); }
    if (a.bad_samples) { fprintf(stderr, "Invalid --samples:\x1b[31m%s\x1b[0m (expected a number of completions, 1 to 16)\n", a.bad_samples); usage(argv[0]); exit(-1); }
    if (a.bad_draft) { fprintf(stderr, "Invalid --draft:\x1b[31m%s\x1b[0m (expected K or K,G with 4 <= K <= 15 and 1 <= G <= 8)\n", a.bad_draft); usage(argv[0]); exit(-1); }
    if (!a.bad_sampling && a.mirostat == 2 && a.typical > 0.0f && a.typical < 1.0f) a.bad_sampling = "--typical together with --mirostat 2";
    if (a.bad_sampling) { fprintf(stderr, "Invalid sampling control:\x1b[31m%s\x1b[0m (--top-k >= 0, --min-p in [0, 1), --repeat-penalty > 0, --repeat-last-n 0..1024, --logit-bias id=val[,id=val...] with at most 256 pairs, --typical a number, --mirostat 0 or 2 with finite --mirostat-ent / --mirostat-lr, never --typical in (0, 1) together with --mirostat 2)\n", a.bad_sampling); usage(argv[0]); exit(-1); }
    if (a.bad_logprobs) { fprintf(stderr, "Invalid --logprobs:\x1b[31m%s\x1b[0m (expected N or N,shaped with 0 <= N <= 20)\n", a.bad_logprobs); usage(argv[0]); exit(-1); }
    if (!a.bad_stop && a.stop_seqs.size() + a.stop_strs.size() > (size_t)FLM_STOP_SEQS_MAX) a.bad_stop = "more than 16 --stop-seq / --stop";
    if (a.bad_stop) { fprintf(stderr, "Invalid stop rule:\x1b[31m%s\x1b[0m (--stop-ids a,b,... with at most 64 distinct ids >= 0; --stop-seq a,b,... with 1 to 32 ids >= 0; --stop a non-empty string; at most 16 sequences and strings)\n", a.bad_stop); usage(argv[0]); exit(-1); }
    if (a.rounds < 1) a.rounds = a.mode == Mode::TEST ? 16 : 1;
}

// --constraint FILE -> CSR arrays sorted by (state, token); false with `why` set for anything that is not the format or breaks a rule of flm_dfa_validate that needs no
// vocabulary (the token bound is checked against the model's once it is loaded)
bool load_constraint(const char* path, Args& a, std::string& why) {
    FILE* f = fopen(path, "r");
    if (!f) { why = "cannot open the file"; return false; }
    char tag[16] = {0}; int ver = 0, ns = 0;
    struct Edge { long q, t, n; };
    std::vector<Edge> edges;
    bool ok = fscanf(f, "%15s %d %d", tag, &ver, &ns) == 3 && !strcmp(tag, "flm-dfa") && ver == 1 && ns >= 1 && ns <= FLM_DFA_STATES_MAX;
    if (!ok) why = "the first line must be `flm-dfa 1 <n_states>` with 1 <= n_states <= 65536";
    while (ok) {
        Edge e; const int got = fscanf(f, "%ld %ld %ld", &e.q, &e.t, &e.n);
        if (got == EOF) break;
        ok = got == 3 && e.q >= 0 && e.q < ns && e.t >= 0 && e.t <= 0x7ffffffe && e.n >= 0 && e.n < ns && edges.size() < (size_t)FLM_DFA_EDGES_MAX;
        if (!ok) why = "every further line must be `state token next` with both states in [0, n_states) and token >= 0";
        else edges.push_back(e);
    }
    fclose(f);
    if (!ok) return false;
    std::sort(edges.begin(), edges.end(), [](const Edge& x, const Edge& y) { return x.q != y.q ? x.q < y.q : x.t < y.t; });
    a.dfa_row.assign(ns + 1, 0);
    for (const Edge& e : edges) { a.dfa_row[e.q + 1] += 1; a.dfa_tok.push_back((int32_t)e.t); a.dfa_nxt.push_back((int32_t)e.n); }
    for (int q = 0; q < ns; ++q) a.dfa_row[q + 1] += a.dfa_row[q];
    flm_dfa d{ns, (int32_t)edges.size(), a.dfa_row.data(), a.dfa_tok.data(), a.dfa_nxt.data()};
    if (flm_dfa_validate(&d, 0x7fffffff) != FLM_OK) { why = flm_last_error(nullptr); return false; }
    return true;
}

int64_t now_us() { return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::high_resolution_clock::now().time_since_epoch()).count(); }

int encode_decode(const Args& a) {                       // main.cpp:246-286
    ModelFile mf; std::string err;
    if (!load_model_file(a.ckpt, a.tknr, FileType::UNKNOWN, true, false, mf, err)) { fprintf(stderr, "Failed to load model\n%s\n", err.c_str()); return -1; }
    Tokenizer tk; tk.set_vocab(std::move(mf.vocab));
    auto show = [](const char* title, const std::vector<int>& v) { print_vector(title, v); };
    if (!a.decode_str.empty()) {
        std::vector<int> toks; const char* s = a.decode_str.c_str();
        while (*s) { if (*s == '-' || (*s >= '0' && *s <= '9')) { char* e; toks.push_back((int)strtol(s, &e, 10)); s = e; } else ++s; }
        show("tokens: ", toks);
        std::cout << "  text: " << tk.decode(toks) << std::endl;
    } else {
        std::cout << "  text: " << a.encode_str << std::endl;
        show("tokens: ", tk.encode(a.encode_str, true));
    }
    return 0;
}
} // namespace

int main(int argc, const char** argv) {
    Args args; parse(args, argc, argv);
    if (!args.encode_str.empty() || !args.decode_str.empty()) return encode_decode(args);
    if (!args.prompt || !args.prompt[0])
        args.prompt = "That was a long long story happened in the ancient Europe. It was about a brave boy name Oliver. Oliver lived in a small village among many big moutains. It was a beautiful village.";
    if (args.detail) {
        fprintf(stderr, "num_threads:%s%d%s\n   use_numa:%s%d%s\n  ckpt_path:%s%s%s\n  tknr_path:%s%s%s\n      top_p:%s%g%s\ntemperature:%s%g%s\n\n",
                Y, args.num_threads, E, Y, (int)args.use_numa, E, Y, args.ckpt.c_str(), E, Y, args.tknr.c_str(), E, Y, args.topp, E, Y, args.temp, E);
    }
    if (args.devices.empty()) args.devices.push_back(args.device);
    // ranks sharing a GPU wait for each other inside their launches: each needs a hardware queue of its own (HIP's default is 4 per process)
    if (args.devices.size() > 1) setenv("GPU_MAX_HW_QUEUES", "16", 0);
    if (args.lookup_k && (args.devices.size() > 1 || args.temp != 0.0f)) {
        fprintf(stderr, "warning: --lookup applies to -t 0 on one device only; ignored\n");
        args.lookup_k = 0;
    }
    if (args.draft_k && args.devices.size() > 1) {
        fprintf(stderr, "warning: --draft applies to one device only; ignored\n");
        args.draft_k = 0;
    }
    if (!args.draft_model.empty() && args.devices.size() > 1) {
        fprintf(stderr, "warning: --draft-model applies to one device only; ignored\n");
        args.draft_model.clear();
    }
    if (args.logprobs_n >= 0 && args.devices.size() > 1) {      // (refused, not ignored: the lines are what the caller asked for)
        fprintf(stderr, "--logprobs applies to one device only: it cannot be combined with --devices of more than one\n");
        return -1;
    }
    const bool stop_set = !args.stop_ids.empty() || !args.stop_seqs.empty() || !args.stop_strs.empty();
    if (args.samples && (args.devices.size() > 1 || args.lookup_k || args.draft_k || !args.draft_model.empty() || args.shape_set || args.ent_set || args.logprobs_n >= 0 || stop_set ||
                         args.constraint || args.mode != Mode::GEN)) {      // (refused, not ignored: flm_generate_n is the plain loop's contract, n times)
        fprintf(stderr, "--samples applies to --mode gen on one device, without --lookup / --draft / --draft-model, the sampling controls, --typical / --mirostat, --logprobs, the stop rules and --constraint\n");
        return -1;
    }
    if (args.prompts_file && (args.samples || args.devices.size() > 1 || args.lookup_k || args.draft_k || !args.draft_model.empty() || args.shape_set || args.ent_set || args.logprobs_n >= 0 || stop_set ||
                              args.constraint || args.mode != Mode::GEN)) {      // (refused, not ignored: flm_generate_batch is the plain loop's contract, once per prompt)
        fprintf(stderr, "--prompts applies to --mode gen on one device, without --samples, --lookup / --draft / --draft-model, the sampling controls, --typical / --mirostat, --logprobs, the stop rules and --constraint\n");
        return -1;
    }
    if (args.batch_rows >= 0 && !args.prompts_file) {          // (refused, not ignored: only flm_generate_batch reads the budget)
        fprintf(stderr, "--batch-rows applies to --prompts only\n");
        return -1;
    }
    if (stop_set && args.devices.size() > 1) {                  // (refused, not ignored: where the output ends is what the caller asked for)
        fprintf(stderr, "--stop-ids / --stop-seq / --stop apply to one device only: they cannot be combined with --devices of more than one\n");
        return -1;
    }
    if (args.constraint) {                  // a malformed file is a usage error, before any model is loaded
        std::string why;
        if (!load_constraint(args.constraint, args, why)) { fprintf(stderr, "Invalid --constraint file:\x1b[31m%s\x1b[0m (%s)\n", args.constraint, why.c_str()); usage(argv[0]); return -1; }
    }
    if (!args.draft_model.empty()) {        // a file that cannot be read is a usage error, before any model is loaded
        FILE* f = fopen(args.draft_model.c_str(), "rb");
        if (!f) { fprintf(stderr, "Invalid --draft-model file:\x1b[31m%s\x1b[0m (cannot open the file)\n", args.draft_model.c_str()); usage(argv[0]); return -1; }
        fclose(f);
    }
    GpuTransformer tf(args.detail || args.debug);
    if (args.constraint) tf.set_constraint(args.dfa_row, args.dfa_tok, args.dfa_nxt);
    if (args.shape_set) tf.set_sampling(args.shape, args.repeat_last_n, args.bias_ids, args.bias_values);
    if (args.ent_set) tf.set_entropy(flm_entropy{args.typical, args.mirostat, args.miro_tau, args.miro_eta, 2.0f * args.miro_tau});
    if (args.logprobs_n >= 0) tf.set_logprobs(args.logprobs_n, args.logprobs_shaped);
    if (stop_set) tf.set_stop(args.stop_ids, args.stop_seqs, args.stop_strs);
    if (args.lookup_k) tf.set_lookup(args.lookup_k, args.lookup_g);
    if (args.draft_k) tf.set_draft(args.draft_k, args.draft_g);
    if (!tf.load(args.ckpt, args.tknr, args.ft, args.qtype, args.devices)) { fprintf(stderr, "Failed to load model\n%s\n", tf.error().c_str()); return 1; }
    if (!args.draft_model.empty() && !tf.load_draft(args.draft_model, args.tknr, args.ft, args.qtype, args.devices[0])) { fprintf(stderr, "Failed to load the draft model\n%s\n", tf.error().c_str()); return 1; }
    args.qtype = tf.get_quant_type();
    if (args.detail) fprintf(stderr, "Model loaded\n\n");

    if (args.mode == Mode::SCORE) {      // (its own lines: the reference has no such mode, and the summary line below stays the reference's)
        if (!tf.score(args.prompt)) { fprintf(stderr, "%s\n", tf.error().c_str()); return 1; }
        return 0;
    }

    if (args.samples) {      // (its own lines: the completions one after another; no summary line -- tools/fan_bench.py times this path)
        std::vector<std::string> texts;
        if (!tf.generate_samples(args.prompt, args.samples, (uint64_t)(int64_t)args.seed, args.max_tokens, args.temp, args.topp, texts)) { fprintf(stderr, "%s\n", tf.error().c_str()); return 1; }
        printf("prompt: %s%s%s\n", Y, args.prompt, E);
        for (size_t j = 0; j < texts.size(); ++j) printf("--- sample %zu ---\n%s\n", j, texts[j].c_str());
        return 0;
    }

    if (args.prompts_file) {      // (its own lines: the completions in the file's order; no summary line -- tools/batch_bench.py times this path's library calls)
        std::vector<std::string> texts;
        if (!tf.generate_prompts(args.prompts, (uint64_t)(int64_t)args.seed, args.max_tokens, args.temp, args.topp, texts, args.batch_rows)) { fprintf(stderr, "%s\n", tf.error().c_str()); return 1; }
        for (size_t j = 0; j < texts.size(); ++j) printf("--- prompt %zu ---\n%s\n", j, texts[j].c_str());
        return 0;
    }

    double sum_prompt_tok = 1e-10, sum_output_tok = 1e-10, sum_prompt_ms = 1e-10, sum_output_ms = 1e-10;
    for (int r = 0; r < args.rounds; ++r) {
        int prompt_tokens = 0, output_tokens = 0; int64_t first_us = 0;
        const int64_t t0 = now_us();
        auto cb = [&](const char* text, int n_in, int n_out, bool ended) -> bool {
            if (first_us == 0) {
                if (args.mode != Mode::TEST) { printf("prompt: %s%s%s\n", Y, args.prompt, E); printf("output: %s", G); }
                first_us = now_us() - t0; prompt_tokens = n_in;
            } else output_tokens = n_out;
            if (args.mode != Mode::TEST && text) { printf("%s", text); fflush(stdout); }
            return !ended;
        };
        if (!tf.generate(args.prompt, cb, args.max_tokens, args.temp, args.topp) && !tf.error().empty()) { fprintf(stderr, "%s\n", tf.error().c_str()); return 1; }
        const int64_t total_us = now_us() - t0;
        if (args.mode != Mode::TEST) printf("%s\n\n", E);
        if (args.mode != Mode::TEST && args.logprobs_n >= 0) {      // --logprobs: index id logprob | id:logprob ...; the log-probability in double from the record's exact ingredients
            const auto& lp = tf.logprobs();
            for (size_t i = 0; i < lp.size(); ++i) {
                printf("%zu %d %.9g |", i, (int)lp[i].token, ((double)lp[i].logit - (double)lp[i].max_logit) - log((double)lp[i].sum));
                for (int j = 0; j < lp[i].n_top; ++j) printf(" %d:%.9g", (int)lp[i].top_id[j], ((double)lp[i].top_logit[j] - (double)lp[i].max_logit) - log((double)lp[i].sum));
                printf("\n");
            }
        }
        if ((args.mode_test || stop_set) && tf.stop_reason() >= 0) {      // the finish reason (flm_query "stop_reason" / "stop_rule"): --mode test, and wherever stop rules were given
            static const char* const kReason[] = {"length", "stop_token", "stop_id", "stop_seq", "cancel"};
            printf("finish_reason:%s\trule:%d\toutput_size:%d\n", kReason[tf.stop_reason() > 4 ? 0 : tf.stop_reason()], tf.stop_rule(), output_tokens);
        }
        sum_prompt_tok += prompt_tokens; sum_output_tok += output_tokens;
        sum_prompt_ms += first_us / 1000.; sum_output_ms += (total_us - first_us) / 1000.;
    }
    const double pt = sum_prompt_tok / args.rounds, ot = sum_output_tok / args.rounds, pm = sum_prompt_ms / args.rounds, om = sum_output_ms / args.rounds;
    const double first_lat = pm / pt, later_lat = om / (ot - 1);
    const char* qn = args.qtype == 2 ? "int8" : args.qtype == 1 ? "int16" : args.qtype == 3 ? "int4" : "None";
    // the reference's summary line (main.cpp:136-145); simd_size reports the wavefront width here
    printf("num_threads:%s%2d%s\tquant:%s%s%s\tuse_numa:%s%d%s\tsimd_size:%d\tprompt_size:%3d\toutput_size:%3d\ttotal_latancy:%5.0fms\t"
           "prompt_token_latancy:%s%4.2f%sms\toutput_token_latancy:%s%4.2f%sms\tprompt_speed:%s%5.1f%stps\toutput_speed:%s%5.1f%stps",
           Y, args.num_threads, E, G, qn, E, G, (int)args.use_numa, E, 64, (int)pt, (int)ot, pm + om,
           Y, first_lat, E, Y, later_lat, E, G, 1000. / first_lat, E, G, 1000. / later_lat, E);
    if (args.lookup_k) printf("\tlookup:%d,%d\taccepted/steps:%s%d/%d%s", args.lookup_k, args.lookup_g, G, tf.lookup_accepted(), tf.lookup_steps(), E);   // (--lookup only: without it the line is the reference's)
    if (!args.draft_model.empty()) printf("\tdraft_model:%d\taccepted/steps:%s%d/%d%s", args.draft_k ? args.draft_k : 7, G, tf.lookup_accepted(), tf.lookup_steps(), E);   // (--draft-model only)
    else if (args.draft_k) printf("\tdraft:%d,%d\taccepted/steps:%s%d/%d%s", args.draft_k, args.draft_g, G, tf.lookup_accepted(), tf.lookup_steps(), E);      // (--draft only)
    printf("\n");
    return 0;
}
