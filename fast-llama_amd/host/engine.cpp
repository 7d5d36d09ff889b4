#include "engine.h"
#include <algorithm>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <chrono>

#include <iomanip>
#include <iostream>
#include <thread>

namespace flmhost {

GpuTransformer::~GpuTransformer() {
    if (_draft_ctx) { if (!_ctxs.empty() && _ctxs[0]) flm_draft_set(_ctxs[0], nullptr); flm_ctx_destroy(_draft_ctx); }      // (detached first: the target does not own it)
    for (flm_ctx* c : _ctxs) if (c) flm_ctx_destroy(c);
}

// --draft-model: a second model on the target's device, in a context of its own, paired with the target (flm_draft_set checks the vocabulary)
bool GpuTransformer::load_draft(const std::string& ckpt, const std::string& tknr, FileType ft, int qtype, int device) {
    if (_ctxs.size() != 1 || !_ctxs[0]) { _err = "--draft-model: one device only, and the model is loaded first"; return false; }
    ModelFile mf;
    if (!load_model_file(ckpt, tknr, ft, false, _debug, mf, _err)) { _err = "--draft-model: " + _err; return false; }
    Config cfg = mf.cfg;
    if (cfg.quant_type == 0) cfg.quant_type = qtype;           // the file's quant type wins over -q, as for the model itself
    flm_model_desc d{};
    d.dim = cfg.dim; d.hidden_dim = cfg.hidden_dim; d.n_layers = cfg.n_layers; d.n_heads = cfg.n_heads; d.n_kv_heads = cfg.n_kv_heads;
    d.vocab_size = cfg.vocab_size; d.max_seq_len = _cfg.max_seq_len; d.quant_type = cfg.quant_type; d.quant_group_size = cfg.quant_group_size;
    if (flm_ctx_create(&d, device, 0, 1, nullptr, &_draft_ctx) != FLM_OK) { _err = std::string("--draft-model: GPU context: ") + flm_last_error(nullptr); _draft_ctx = nullptr; return false; }
    for (const HostTensor& t : mf.tensors)
        if (flm_upload_tensor(_draft_ctx, t.kind, t.layer, t.qtype, t.values, t.scales, t.rows, t.cols) != FLM_OK) { _err = std::string("--draft-model: upload: ") + flm_last_error(_draft_ctx); return false; }
    if (flm_draft_set(_ctxs[0], _draft_ctx) != FLM_OK) { _err = std::string("--draft-model: ") + flm_last_error(_ctxs[0]); flm_ctx_destroy(_draft_ctx); _draft_ctx = nullptr; return false; }
    return true;
}

int GpuTransformer::on_all(const std::function<int(int)>& f) {
    const int n = (int)_ctxs.size();
    if (n == 1) return f(0);
    std::vector<int> rc(n, 0);
    std::vector<std::thread> th;
    for (int r = 1; r < n; ++r) th.emplace_back([&, r] { rc[r] = f(r); });
    rc[0] = f(0);
    for (auto& t : th) t.join();
    for (int r = 0; r < n; ++r) if (rc[r] != FLM_OK) { _err = std::string("rank ") + std::to_string(r) + ": " + flm_last_error(_ctxs[r]); return rc[r]; }
    return FLM_OK;
}

bool GpuTransformer::load(const std::string& ckpt, const std::string& tknr, FileType ft, int qtype, const std::vector<int>& devices, uint64_t seed) {
    ModelFile mf;
    if (!load_model_file(ckpt, tknr, ft, false, _debug, mf, _err)) return false;
    _cfg = mf.cfg;
    _cfg.max_seq_len = 1024;                                   // transformer.cpp:32
    if (_cfg.quant_type == 0) _cfg.quant_type = qtype;         // the file's quant type wins over -q (transformer.cpp:36-38)
    _tok.set_vocab(std::move(mf.vocab));
    _sampler.build(_cfg.vocab_size, seed);
    flm_model_desc d{};
    d.dim = _cfg.dim; d.hidden_dim = _cfg.hidden_dim; d.n_layers = _cfg.n_layers; d.n_heads = _cfg.n_heads; d.n_kv_heads = _cfg.n_kv_heads;
    d.vocab_size = _cfg.vocab_size; d.max_seq_len = _cfg.max_seq_len; d.quant_type = _cfg.quant_type; d.quant_group_size = _cfg.quant_group_size;
    const int world = (int)devices.size();
    if (world < 1 || world > 8) { _err = "1 to 8 devices"; return false; }
    _ctxs.assign(world, nullptr);
    for (int r = 0; r < world; ++r) {
        const int rc = flm_ctx_create(&d, devices[r], r, world, nullptr, &_ctxs[r]);
        if (rc != FLM_OK) { _err = std::string("GPU context (rank ") + std::to_string(r) + ", device " + std::to_string(devices[r]) + "): " + flm_last_error(nullptr); return false; }
    }
    for (const HostTensor& t : mf.tensors) {
        // a quantized tensor of another type than the model's cannot be multiplied (tensor.cpp:557-561); every rank is handed the full tensor and keeps its rows
        for (int r = 0; r < world; ++r) {
            const int rc = flm_upload_tensor(_ctxs[r], t.kind, t.layer, t.qtype, t.values, t.scales, t.rows, t.cols);
            if (rc != FLM_OK) { _err = std::string("upload: ") + flm_last_error(_ctxs[r]); return false; }
        }
    }
    if (world > 1) {
        if (!connect_ranks()) return false;
        if (!calibrate_structure()) return false;
    }
    return true;
}

// connect the ranks peer to peer: every rank's exchange buffer mapped into every other (ranks of one process share pointers); also the round at which the group
// agrees on its launch structure from every rank's options
bool GpuTransformer::connect_ranks() {
    const int world = (int)_ctxs.size();
    std::vector<unsigned char> blobs((size_t)world * FLM_P2P_BLOB_BYTES);
    for (int r = 0; r < world; ++r)
        if (flm_p2p_export(_ctxs[r], blobs.data() + (size_t)r * FLM_P2P_BLOB_BYTES) != FLM_OK) { _err = std::string("p2p export: ") + flm_last_error(_ctxs[r]); return false; }
    for (int r = 0; r < world; ++r)
        if (flm_p2p_import(_ctxs[r], blobs.data(), world) != FLM_OK) { _err = std::string("p2p import: ") + flm_last_error(_ctxs[r]); return false; }
    return true;
}

// The group's launch structure.  Default: what the LIBRARY takes by itself -- between distinct devices the conservative structure (a flag round behind a kernel boundary, release /
// acquire fences), on one device the folded / rank-spanning launches.  The faster structures between devices rely on system-scope store / flag ordering over xGMI that the build box could
// only rehearse between CU partitions of one GPU, and a memory-ordering race is rare: one matching token verifies nothing.  They are therefore OPT-IN (FLM_TP_CALIBRATE=1 in the
// environment): every candidate must then reproduce the conservative structure's ids over a 96-token greedy decode AND its last logits bit for bit on every rank, is timed on the
// device (flm_decode_timed: HIP events, median of three runs of 32 tokens) and replaces the incumbent only if at least 2 % faster.  A candidate that fails in any way other than a
// mismatch (a time-out raises the group's abort line on every peer: the contexts cannot be used any more) is fatal -- load() fails instead of returning a poisoned group.
bool GpuTransformer::calibrate_structure() {
    const char* env = getenv("FLM_TP_CALIBRATE");
    if (!env || !env[0] || env[0] == '0') { _tp_structure = "library default"; return true; }
    struct Cand { const char* name; int trust, ffn, layers, fence, gr; };
    const Cand cands[] = {{"exchange launches", 0, 0, 0, -1, 0}, {"folded exchanges, QKV + attention + Wo across ranks", 1, 0, 0, -1, 0},
                          {"all layers in one rank-spanning launch, fenced flags", 1, 0, 1, 3, 0}, {"all layers in one rank-spanning launch, flags", 1, 0, 1, 0, 0},
                          {"all layers in one rank-spanning launch, data-tagged granules (no flag, no fence)", 1, 0, 1, -1, 1},
                          {"folded exchanges, + FFN13 + FFN2 across ranks", 1, 1, 0, -1, 0}};
    const int world = (int)_ctxs.size(), V = _cfg.vocab_size, kVerify = 96 < _cfg.max_seq_len - 2 ? 96 : _cfg.max_seq_len - 2, kTime = kVerify < 32 ? kVerify : 32;
    auto apply = [&](const Cand& c) {
        for (int r = 0; r < world; ++r)
            if (flm_set_option(_ctxs[r], "tp_trust_fused", c.trust) != FLM_OK || flm_set_option(_ctxs[r], "tp_fuse_ffn", c.ffn) != FLM_OK ||
                flm_set_option(_ctxs[r], "tp_fuse_layers", c.layers) != FLM_OK || flm_set_option(_ctxs[r], "tp_fence", c.fence) != FLM_OK || flm_set_option(_ctxs[r], "gr_edges", c.gr) != FLM_OK) { _err = std::string("set_option: ") + flm_last_error(_ctxs[r]); return false; }
        return connect_ranks();
    };
    // BOS at position 0, then kVerify greedy tokens: every rank's ids and its last logits are the verdict; then the device time of kTime tokens (median of three)
    struct Probe { std::vector<int32_t> ids; std::vector<float> logits; double us = 0.0; };
    auto probe = [&](Probe& p) -> int {     // 0 ok, 1 the ranks disagree among themselves, -1 an error (fatal for the group)
        std::vector<std::vector<int32_t>> ids(world, std::vector<int32_t>(kVerify));
        std::vector<std::vector<float>> lg(world, std::vector<float>(V));
        const int32_t tok = 1;
        if (on_all([&](int r) { return flm_reset_kv(_ctxs[r]); }) != FLM_OK) return -1;
        if (on_all([&](int r) { int rc = flm_decode_greedy(_ctxs[r], tok, 0, kVerify, ids[r].data()); if (rc == FLM_OK) rc = flm_forward(_ctxs[r], &ids[r][kVerify - 1], 1, kVerify, lg[r].data()); return rc; }) != FLM_OK) return -1;
        for (int r = 0; r < world; ++r) { int fb = 0; flm_query(_ctxs[r], "fallback", &fb); if (fb) { _err = "a cross-workgroup wait timed out"; return -1; } }
        for (int r = 1; r < world; ++r) if (ids[r] != ids[0] || memcmp(lg[r].data(), lg[0].data(), (size_t)V * 4) != 0) return 1;
        std::vector<double> t;
        for (int rep = 0; rep < 3; ++rep) {
            std::vector<float> ms(world, 0.f);
            if (on_all([&](int r) { return flm_decode_timed(_ctxs[r], tok, 0, kTime, &ms[r]); }) != FLM_OK) return -1;
            double m = 0; for (float x : ms) if (x > m) m = x;
            t.push_back(m * 1000.0 / kTime);
        }
        std::sort(t.begin(), t.end());
        p.ids = ids[0]; p.logits = lg[0]; p.us = t[1];
        return 0;
    };
    Probe want, got;
    int best = 0;
    if (!apply(cands[0])) return false;
    if (probe(want) != 0) { if (_err.empty()) _err = "tensor parallel: the conservative structure does not give the same results on every rank"; return false; }
    double best_us = want.us;
    for (int i = 1; i < (int)(sizeof cands / sizeof cands[0]); ++i) {
        if (!apply(cands[i])) return false;
        const int rc = probe(got);
        if (rc < 0) { if (_err.empty()) _err = std::string("tensor parallel: structure \"") + cands[i].name + "\" failed: " + flm_last_error(_ctxs[0]); return false; }   // (the group may be poisoned: no way back)
        if (rc > 0 || got.ids != want.ids || memcmp(got.logits.data(), want.logits.data(), (size_t)V * 4) != 0) {
            if (_debug) fprintf(stderr, "tensor parallel: structure \"%s\" dropped (its ids / logits differ from the conservative structure's)\n", cands[i].name);
            continue;
        }
        if (_debug) fprintf(stderr, "tensor parallel: structure \"%s\": %.1f us per token against %.1f\n", cands[i].name, got.us, best_us);
        if (got.us < 0.98 * best_us) { best_us = got.us; best = i; }
    }
    if (!apply(cands[best])) return false;
    _tp_structure = cands[best].name;
    return on_all([&](int r) { return flm_reset_kv(_ctxs[r]); }) == FLM_OK;
}

std::vector<int> GpuTransformer::encode(const char* prompt) const {
    if (!prompt || !prompt[0]) return {};
    auto v = _tok.encode(prompt, true);
    if ((int)v.size() > _cfg.max_seq_len) v.resize(_cfg.max_seq_len);
    return v;
}

void print_vector(const char* title, const std::vector<int>& vec) {       // utility.cpp:67-94
    int dw = 1;
    if (!vec.empty()) {
        int mn = vec[0], mx = vec[0];
        for (int v : vec) { if (v > mx) mx = v; else if (v < mn) mn = v; }
        for (int v = 10; v <= mx; v *= 10, ++dw) {}
        if (mn < 0 && -mn > mx) { dw = 2; for (int v = -10; v >= mn; v *= 10, ++dw) {} }
    }
    std::cout << title << "[";
    for (size_t i = 0; i < vec.size(); ++i) { if (i) std::cout << ", "; std::cout << std::setw(dw) << vec[i]; }
    std::cout << "]" << std::endl;
}

bool GpuTransformer::score(const char* prompt) {
    const std::vector<int> input = encode(prompt);
    if (input.empty()) { fprintf(stderr, "Empty input for score()\n"); return false; }
    if (_ctxs.size() != 1) { _err = "score: one device only"; return false; }
    printf("Input prompt:%s\n", prompt);
    print_vector("Input tokens:", input);
    const int n = (int)input.size();
    std::vector<flm_score> sc(n);
    const auto t0 = std::chrono::high_resolution_clock::now();
    const int rc = flm_score_tokens(_ctxs[0], input.data(), n, 0, nullptr, sc.data(), nullptr);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
    if (rc != FLM_OK) { _err = std::string("score: ") + flm_last_error(_ctxs[0]); return false; }
    // the unclipped log-probability from the row's exact ingredients, in double: (target_logit - max_logit) - log(sum); the last row has no target
    double loss = 0.0;
    for (int i = 0; i < n; ++i) {
        printf("score:%4d\ttoken:%6d\targmax:%6d\tprob:%.9g\n", i, input[i], (int)sc[i].argmax, (double)sc[i].prob);
        if (i + 1 < n) loss -= ((double)sc[i].target_logit - (double)sc[i].max_logit) - log((double)sc[i].sum);
    }
    const double mean = n > 1 ? loss / (n - 1) : 0.0;
    printf("score_tokens:%3d\tmean_loss:%.6f\tperplexity:%.4f\tscore_latancy:%5.2fms\n", n, mean, exp(mean), ms);
    return true;
}

bool GpuTransformer::generate_samples(const char* prompt, int n, uint64_t seed, int max_new_tokens, float temperature, float topp, std::vector<std::string>& texts) {
    texts.clear();
    if (_ctxs.size() != 1) { _err = "--samples: one device only"; return false; }
    if (n < 1 || n > FLM_FAN_MAX) { _err = "--samples: 1 to 16 samples"; return false; }
    const std::vector<int> input = encode(prompt);
    if (input.empty()) { fprintf(stderr, "Empty input for generate()\n"); return false; }
    printf("Input prompt:%s\n", prompt);
    print_vector("Input tokens:", input);
    const int n_in = (int)input.size();
    if (n_in >= _cfg.max_seq_len) { fprintf(stderr, "Input is too long for generate()\n"); return false; }
    if (max_new_tokens < 0) max_new_tokens = 0;
    if (max_new_tokens > (_cfg.max_seq_len - n_in) / n) max_new_tokens = (_cfg.max_seq_len - n_in) / n;      // (the n tails share what the prompt leaves: flm_fan_layout_for)
    const int want = max_new_tokens + 1;
    std::vector<int32_t> ids((size_t)n * want);
    std::vector<int> n_out(n, 0);
    std::vector<uint64_t> st(n);
    for (int j = 0; j < n; ++j) st[j] = seed + (uint64_t)j;
    const int rc = n == 1 ? flm_generate(_ctxs[0], input.data(), n_in, 0, want, temperature, topp, st.data(), 0, nullptr, nullptr, ids.data(), n_out.data())
                          : flm_generate_n(_ctxs[0], input.data(), n_in, 0, want, n, temperature, topp, st.data(), 0, nullptr, nullptr, ids.data(), n_out.data());
    if (rc != FLM_OK) { _err = std::string("--samples: ") + flm_last_error(_ctxs[0]); return false; }
    texts.resize(n);
    for (int j = 0; j < n; ++j) {
        int prev = -1;
        for (int i = 0; i < n_out[j]; ++i) { const int tok = ids[(size_t)j * want + i]; texts[j] += _tok.decode(tok, prev); prev = tok; }
    }
    return true;
}

bool GpuTransformer::generate_prompts(const std::vector<std::string>& prompts, uint64_t seed, int max_new_tokens, float temperature, float topp, std::vector<std::string>& texts, int batch_rows) {
    texts.clear();
    const int n = (int)prompts.size();
    if (_ctxs.size() != 1) { _err = "--prompts: one device only"; return false; }
    if (n < 1 || n > FLM_BATCH_MAX) { _err = "--prompts: 1 to 16 prompts"; return false; }
    if (max_new_tokens < 0) max_new_tokens = 0;
    const int share = _cfg.max_seq_len / n;                  // (every prompt gets an equal share of the cache's rows: flm_batch_layout_for)
    std::vector<std::vector<int>> inputs(n);
    std::vector<flm_batch_req> reqs(n);
    int want = 1;
    for (int j = 0; j < n; ++j) {
        inputs[j] = encode(prompts[j].c_str());
        if (inputs[j].empty()) { fprintf(stderr, "Empty input for generate()\n"); return false; }
        printf("Input prompt:%s\n", prompts[j].c_str());
        print_vector("Input tokens:", inputs[j]);
        const int n_in = (int)inputs[j].size();
        if (n_in >= share) { fprintf(stderr, "Input is too long for generate()\n"); return false; }
        const int room = share - n_in;
        flm_batch_req& q = reqs[j];
        q.prompt = inputs[j].data(); q.n_prompt = n_in; q.max_tokens = (max_new_tokens < room ? max_new_tokens : room) + 1;
        q.temperature = temperature; q.topp = topp; q.rng_state = seed + (uint64_t)j; q.stop_token = 0;
        want = q.max_tokens > want ? q.max_tokens : want;
    }
    std::vector<int32_t> ids((size_t)n * want);
    std::vector<int> n_out(n, 0);
    if (flm_set_option(_ctxs[0], "batch_rows", batch_rows < 0 ? -1 : batch_rows) != FLM_OK) { _err = std::string("--batch-rows: ") + flm_last_error(_ctxs[0]); return false; }
    const int rc = flm_generate_batch(_ctxs[0], reqs.data(), n, nullptr, nullptr, ids.data(), want, n_out.data(), nullptr);
    if (rc != FLM_OK) { _err = std::string("--prompts: ") + flm_last_error(_ctxs[0]); return false; }
    texts.resize(n);
    for (int j = 0; j < n; ++j) {
        int prev = -1;
        for (int i = 0; i < n_out[j]; ++i) { const int tok = ids[(size_t)j * want + i]; texts[j] += _tok.decode(tok, prev); prev = tok; }
    }
    return true;
}

bool GpuTransformer::generate(const char* prompt, const std::function<bool(const char*, int, int, bool)>& cb,
                              int max_new_tokens, float temperature, float topp) {
    const std::vector<int> input = encode(prompt);
    if (input.empty()) { fprintf(stderr, "Empty input for generate()\n"); return false; }
    if (_shape_set) {       // the bias ids against THIS model's vocabulary, here and not only in the C ABI: the host loop below hands them to shape_logits directly
        for (size_t i = 0; i < _bias_ids.size(); ++i) {
            bool bad = _bias_ids[i] < 0 || _bias_ids[i] >= _cfg.vocab_size;
            for (size_t k = 0; k < i && !bad; ++k) bad = _bias_ids[k] == _bias_ids[i];
            if (bad) { _err = "--logit-bias: an id outside [0, vocab) or listed twice"; return false; }
        }
    }
    flm_dfa dfa{};
    if (_dfa_set) {         // against THIS model's vocabulary, here and not only in flm_constraint_set: the host loop below walks the arrays directly
        dfa.n_states = (int32_t)_dfa_row.size() - 1; dfa.n_edges = (int32_t)_dfa_tok.size();
        dfa.row_ptr = _dfa_row.data(); dfa.edge_token = _dfa_tok.data(); dfa.edge_next = _dfa_nxt.data();
        if (flm_dfa_validate(&dfa, _cfg.vocab_size) != FLM_OK) { _err = std::string("--constraint: ") + flm_last_error(nullptr); return false; }
    }
    printf("Input prompt:%s\n", prompt);
    print_vector("Input tokens:", input);
    const int n_in = (int)input.size();
    if (n_in >= _cfg.max_seq_len) { fprintf(stderr, "Input is too long for generate()\n"); return false; }
    if (max_new_tokens > _cfg.max_seq_len - n_in) max_new_tokens = _cfg.max_seq_len - n_in;
    const int max_tokens = n_in + max_new_tokens;

    _lp.clear();
    _stop_reason = -1; _stop_rule = 0;
    if (_stop_set && _ctxs.size() != 1) { _err = "--stop-ids / --stop-seq / --stop: one device only"; fprintf(stderr, "%s\n", _err.c_str()); return false; }
    if (_stop_set && !_stop_installed) {        // the rules, once: the ids, the sequences, then every --stop string's one tokenisation (no BOS); checked against THIS model's vocabulary by flm_stop_set
        std::vector<int32_t> ptr{0}, toks;
        auto add = [&](const std::vector<int32_t>& q) { toks.insert(toks.end(), q.begin(), q.end()); ptr.push_back((int32_t)toks.size()); };
        for (const auto& q : _stop_seqs) add(q);
        for (const auto& str : _stop_strs) { const std::vector<int> e = _tok.encode(str, false); add(std::vector<int32_t>(e.begin(), e.end())); }
        flm_stop_rules sr{(int32_t)_stop_ids.size(), _stop_ids.data(), (int32_t)ptr.size() - 1, ptr.data(), toks.data()};
        if (flm_stop_set(_ctxs[0], &sr) != FLM_OK) { _err = std::string("stop rules: ") + flm_last_error(_ctxs[0]); fprintf(stderr, "%s\n", _err.c_str()); return false; }
        _stop_installed = true;
    }
    if (_lp_top_n >= 0 && _ctxs.size() != 1) { _err = "--logprobs: one device only"; fprintf(stderr, "%s\n", _err.c_str()); return false; }
    if (_lp_top_n >= 0 && _ent_set) { _err = "--logprobs cannot be combined with --typical / --mirostat (not built)"; fprintf(stderr, "%s\n", _err.c_str()); return false; }
    int prev = -1;
    auto emit = [&](int tok, int index, int n_cur) {
        const std::string piece = _tok.decode(tok, prev);
        prev = tok;
        return cb(piece.c_str(), n_in, index + n_cur - n_in, tok == 0);
    };
    std::vector<float> logits(_cfg.vocab_size);
    // the reference's loop (transformer.cpp:91-101): forward at position i, sample, callback, stop on token 0
    int i = 0, next = -1;
    std::vector<int> cur = input;
    const bool greedy = temperature == 0.0f;
    bool dev_sample = !greedy;              // sampled tokens on the device (flm_forward_sample / flm_decode_sample); the host sampler where the library refuses
    const int world = (int)_ctxs.size();
    // the ranks sample identical logits with identical states: their ids and states must agree
    auto agree = [&](const std::vector<std::vector<int32_t>>& ids, const std::vector<uint64_t>& st) {
        for (int r = 1; r < world; ++r) if (ids[r] != ids[0] || st[r] != st[0]) { _err = "tensor parallel: the ranks sampled different tokens"; fprintf(stderr, "%s\n", _err.c_str()); return false; }
        return true;
    };
    if (world == 1) {
        // one device: the whole loop is ONE call (flm_generate): the prompt and every decode token go onto the stream at once, the device stops on token 0 itself and hands
        // each token over as it appears -- text streams per token as the reference's does, nothing is computed past the stop.  The loop's count: one token from the prompt,
        // then one per position up to max_tokens (the arithmetic above).  The host-sampler loop below stays for vocabularies the device sampler refuses.
        struct Sink { decltype(emit)* fn; int n_in; } sink{&emit, n_in};
        const flm_token_cb on_token = [](void* user, int index, int32_t token, int /*last*/) -> int {
            Sink* s = (Sink*)user;
            return (*s->fn)(token, index == 0 ? 0 : s->n_in + index - 1, index == 0 ? s->n_in : 1) ? 0 : 1;      // (emit's false: cancel)
        };
        uint64_t st = _sampler.state();
        int n_out = 0;
        const int want = (max_new_tokens > 0 ? max_new_tokens : 0) + 1;
        int rc = FLM_ERR_UNSUPPORTED;
        bool whole = true;                  // the plain loop (flm_generate) still has to run
        auto count = [&] {
            int v = 0;
            if (rc == FLM_OK && flm_query(_ctxs[0], "spec_steps", &v) == FLM_OK) _lookup_steps += v;
            if (rc == FLM_OK && flm_query(_ctxs[0], "spec_accepted", &v) == FLM_OK) _lookup_accepted += v;
        };
        bool armed = false;                 // --constraint: installed once, armed at state 0 before every run; refused (nothing was launched): the host loop below masks
        if (_dfa_set) {
            int cr = _dfa_installed ? FLM_OK : flm_constraint_set(_ctxs[0], &dfa);
            if (cr == FLM_OK) { _dfa_installed = true; cr = flm_constraint_arm(_ctxs[0], 0); }
            if (cr != FLM_OK && cr != FLM_ERR_UNSUPPORTED) { _err = std::string("--constraint: ") + flm_last_error(_ctxs[0]); fprintf(stderr, "%s\n", _err.c_str()); return false; }
            armed = cr == FLM_OK;
        }
        const bool dev_ok = !_dfa_set || armed;
        const bool lp = _lp_top_n >= 0;     // --logprobs: armed before every run; the records exist on the device path only, so a refusal is an error, not a host loop
        if (lp && (!dev_ok || flm_logprobs_arm(_ctxs[0], _lp_top_n, _lp_shaped ? FLM_LOGPROBS_SHAPED : FLM_LOGPROBS_RAW) != FLM_OK)) {
            _err = std::string("--logprobs: ") + (dev_ok ? flm_last_error(_ctxs[0]) : "the constraint could not be armed on the device"); fprintf(stderr, "%s\n", _err.c_str()); return false;
        }
        bool ent_dev = false;               // --typical / --mirostat: set before every run (Mirostat's state starts over); refused as unsupported: the host loop below runs the stages
        if (_ent_set && dev_ok) {
            const int er = flm_entropy_set(_ctxs[0], &_ent);
            if (er != FLM_OK && er != FLM_ERR_UNSUPPORTED) { _err = std::string("--typical / --mirostat: ") + flm_last_error(_ctxs[0]); fprintf(stderr, "%s\n", _err.c_str()); return false; }
            ent_dev = er == FLM_OK;
        }
        if (_stop_set && _ent_set && !ent_dev) { _err = "--stop-ids / --stop-seq / --stop need the device loop, and --typical / --mirostat could not be set there (the library refused: a vocabulary beyond the device sampler): drop one of the two"; fprintf(stderr, "%s\n", _err.c_str()); return false; }
        if (_stop_set && !dev_ok) { _err = "--stop-ids / --stop-seq / --stop need the device loop, and --constraint could not be installed there (the library refused the automaton): drop one of the two"; fprintf(stderr, "%s\n", _err.c_str()); return false; }
        if (_ent_set && !ent_dev) { whole = false; rc = FLM_ERR_UNSUPPORTED; }
        else if (dev_ok && (_shape_set || armed || lp || _stop_set || ent_dev)) {          // the sampling controls / the constraint: the same loop with the shaping stage on the device (flm_generate_ex; no control flag: neutral controls, masking only); refused: the host loop below shapes
            flm_sampling sp{};
            sp.temperature = temperature; sp.topp = topp; sp.top_k = _shape.top_k; sp.min_p = _shape.min_p; sp.repeat_penalty = _shape.repeat_penalty;
            sp.frequency_penalty = _shape.frequency_penalty; sp.presence_penalty = _shape.presence_penalty; sp.penalty_last_n = _shape_last_n;
            sp.n_bias = _shape.n_bias; sp.bias_ids = _shape.bias_ids; sp.bias_values = _shape.bias_values;
            // with --draft (any temperature) / --lookup (temperature 0): the same ids through draft-and-verify steps whose rows are shaped each over its own window
            // (flm_generate_lookup_ex); refused as unsupported (nothing was launched): the token loop
            if (_draft_ctx) {       // --draft-model: the same ids with the draft model as the drafter (flm_generate_draft), at any temperature
                rc = flm_generate_draft(_ctxs[0], input.data(), n_in, 0, want, &sp, &st, 0, _draft_k > 0 ? _draft_k : 7, on_token, &sink, nullptr, &n_out);
                count();
            }
            else if (_draft_k > 0 || (greedy && _lookup_k > 0)) {
                const bool draft = _draft_k > 0;
                rc = flm_generate_lookup_ex(_ctxs[0], input.data(), n_in, 0, want, &sp, &st, 0, draft ? _draft_k : _lookup_k, draft ? _draft_g : _lookup_g, on_token, &sink, nullptr, &n_out);
                count();
            }
            if (rc == FLM_ERR_UNSUPPORTED) rc = flm_generate_ex(_ctxs[0], input.data(), n_in, 0, want, &sp, &st, 0, on_token, &sink, nullptr, &n_out);
            if (rc == FLM_ERR_INVALID) { _err = flm_last_error(_ctxs[0]); fprintf(stderr, "%s\n", _err.c_str()); }
            if (_stop_set && rc != FLM_OK) { if (_err.empty()) _err = std::string("stop rules: ") + flm_last_error(_ctxs[0]); return false; }      // (the rules live on the device path only)
            if (lp && rc != FLM_OK) { if (_err.empty()) _err = std::string("--logprobs: ") + flm_last_error(_ctxs[0]); return false; }
            if (lp && n_out > 0) {
                _lp.resize((size_t)n_out);
                if (flm_last_logprobs(_ctxs[0], 0, n_out, _lp.data()) != FLM_OK) { _err = std::string("--logprobs: ") + flm_last_error(_ctxs[0]); _lp.clear(); return false; }
            }
            whole = false;
        } else if (dev_ok && _draft_ctx) {
            // --draft-model: the plain loop's ids through draft-and-verify steps drafted by the draft model; refused as unsupported (nothing was launched): the run without the flag
            flm_sampling sp{};
            sp.temperature = temperature; sp.topp = topp; sp.repeat_penalty = 1.0f;
            rc = flm_generate_draft(_ctxs[0], input.data(), n_in, 0, want, &sp, &st, 0, _draft_k > 0 ? _draft_k : 7, on_token, &sink, nullptr, &n_out);
            count();
            whole = rc == FLM_ERR_UNSUPPORTED;
        } else if (dev_ok && (_draft_k > 0 || (greedy && _lookup_k > 0))) {
            // --draft: the same loop through draft-and-verify steps at the run's temperature; refused (nothing was launched): the run without the flag.
            // --lookup: the same at temperature 0 only (the same ids and callbacks)
            const bool draft = _draft_k > 0;
            rc = flm_generate_lookup_sample(_ctxs[0], input.data(), n_in, 0, want, temperature, topp, &st, 0, draft ? _draft_k : _lookup_k, draft ? _draft_g : _lookup_g, on_token, &sink, nullptr, &n_out);
            count();
            whole = draft && rc == FLM_ERR_UNSUPPORTED;
        }
        if (!dev_ok || (_ent_set && !ent_dev)) { whole = false; rc = FLM_ERR_UNSUPPORTED; }
        if (whole) rc = flm_generate(_ctxs[0], input.data(), n_in, 0, want, temperature, topp, &st, 0, on_token, &sink, nullptr, &n_out);
        if (rc == FLM_OK) {
            if (!greedy) _sampler.set_state(st);
            if (flm_query(_ctxs[0], "stop_reason", &_stop_reason) != FLM_OK || flm_query(_ctxs[0], "stop_rule", &_stop_rule) != FLM_OK) _stop_reason = -1;
            return true;
        }
        if (rc != FLM_ERR_UNSUPPORTED) return false;
        dev_sample = false;
    }
    // the sampling controls where the loop is the host's: the logits come back, shape_logits runs over the window (the last penalty_last_n ids of the prompt and what was
    // generated since), then the host sampler -- what flm_generate_ex computes on the device
    const bool shaped = _shape_set || _dfa_set || _ent_set;
    float mu = _ent.mu;                     // --mirostat on the host: the running state, from its start
    int q = 0;                              // --constraint on the host: the automaton's state, from 0
    std::vector<int32_t> history;
    if (shaped) history.assign(input.begin(), input.end());
    std::vector<float> shaped_row(shaped ? _cfg.vocab_size : 0);
    if (shaped) dev_sample = false;
    while (next != 0 && i < max_tokens) {
        if (dev_sample && (int)cur.size() == 1) {
            // the device-resident sampled loop, in chunks like the greedy one; the host's Sampler keeps the authoritative state
            int chunk = max_tokens - i; if (chunk > 8) chunk = 8;
            std::vector<std::vector<int32_t>> outs(world, std::vector<int32_t>(chunk));
            std::vector<uint64_t> st(world, _sampler.state());
            const int rc = on_all([&](int r) { return flm_decode_sample(_ctxs[r], cur[0], i, chunk, temperature, topp, &st[r], outs[r].data()); });
            if (rc == FLM_ERR_UNSUPPORTED) { dev_sample = false; continue; }
            if (rc != FLM_OK || !agree(outs, st)) return false;
            _sampler.set_state(st[0]);
            bool stop = false;
            for (int k = 0; k < chunk && !stop; ++k) {
                next = outs[0][k];
                if (!emit(next, i, 1)) stop = true;
                i += 1; cur = {next};
                if (next == 0) stop = true;
            }
            if (stop) break;
            continue;
        }
        if (greedy && !shaped && (int)cur.size() == 1) {
            // temperature 0: run a chunk of tokens in the device-resident greedy loop (no per-token host round trip)
            int chunk = max_tokens - i; if (chunk > 8) chunk = 8;
            std::vector<int32_t> out(chunk);
            std::vector<std::vector<int32_t>> outs(_ctxs.size(), std::vector<int32_t>(chunk));
            if (on_all([&](int r) { return flm_decode_greedy(_ctxs[r], cur[0], i, chunk, outs[r].data()); }) != FLM_OK) return false;
            out = outs[0];
            bool stop = false;
            for (int k = 0; k < chunk && !stop; ++k) {
                next = out[k];
                if (!emit(next, i, 1)) stop = true;
                i += 1; cur = {next};
                if (next == 0) stop = true;
            }
            if (stop) break;
            continue;
        }
        int rc;
        if (greedy && !shaped) {
            std::vector<int32_t> ts(_ctxs.size(), 0);
            rc = on_all([&](int r) { return flm_forward_argmax(_ctxs[r], cur.data(), (int)cur.size(), i, &ts[r]); }); next = ts[0];
        } else if (dev_sample) {
            std::vector<std::vector<int32_t>> ts(world, std::vector<int32_t>(1, 0));
            std::vector<uint64_t> st(world, _sampler.state());
            rc = on_all([&](int r) { return flm_forward_sample(_ctxs[r], cur.data(), (int)cur.size(), i, temperature, topp, &st[r], &ts[r][0]); });
            if (rc == FLM_ERR_UNSUPPORTED) { dev_sample = false; continue; }
            if (rc == FLM_OK && !agree(ts, st)) return false;
            if (rc == FLM_OK) { _sampler.set_state(st[0]); next = ts[0][0]; }
        } else {
            std::vector<std::vector<float>> lgs(_ctxs.size());
            for (size_t r = 1; r < lgs.size(); ++r) lgs[r].resize(_cfg.vocab_size);
            rc = on_all([&](int r) { return flm_forward(_ctxs[r], cur.data(), (int)cur.size(), i, r == 0 ? logits.data() : lgs[r].data()); });
            if (rc == FLM_OK && shaped) {
                const int w = (int)history.size() < _shape_last_n ? (int)history.size() : _shape_last_n;
                if (_dfa_set) constrain_logits(logits.data(), _cfg.vocab_size, _dfa_tok.data() + _dfa_row[q], _dfa_row[q + 1] - _dfa_row[q], logits.data());      // step 0, in place
                shape_logits(logits.data(), _cfg.vocab_size, temperature, _shape, history.data() + (history.size() - w), w, shaped_row.data());
                const bool miro = _ent_set && _ent.mirostat == 2 && temperature != 0.0f;
                if (_ent_set) entropy_logits(shaped_row.data(), _cfg.vocab_size, temperature, _ent.typical_p, _ent.mirostat, mu, shaped_row.data());      // stages 5 / 6, in place
                std::vector<float> masked;
                if (miro) masked = shaped_row;          // (the sampler overwrites its row: the update reads the masked logits)
                next = _sampler.sample(shaped_row.data(), temperature, miro ? 1.0f : topp);
                if (miro) mu = mirostat_update(masked.data(), _cfg.vocab_size, temperature, next, _ent.tau, _ent.eta, mu, nullptr);
                if (_dfa_set) q = dfa_next(_dfa_row.data(), _dfa_tok.data(), _dfa_nxt.data(), q, next);
                history.push_back(next);
            } else if (rc == FLM_OK) next = _sampler.sample(logits.data(), temperature, topp);
        }
        if (rc != FLM_OK) return false;
        if (!emit(next, i, (int)cur.size())) break;
        i += (int)cur.size();
        cur = {next};
    }
    return true;
}

} // namespace flmhost
