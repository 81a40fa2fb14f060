// extern "C" implementation of include/mi_engine.h (the op-level mi_op_* entry points: ops.cpp).
// Every entry point catches exceptions and reports them through mi_last_error().
#include "engine.h"

#include <dlfcn.h>
#include <execinfo.h>
#include <fcntl.h>
#include <signal.h>
#include <rccl/rccl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace mi;

struct mi_model { Model impl; };
struct mi_ctx { std::unique_ptr<Ctx> impl; };
struct mi_lora { std::shared_ptr<Lora> impl; };

// ---- replicas: fill the arenas of header-only models (no_upload) from a loaded one ----
// Weights cross devices by one RCCL broadcast over xGMI (single process: ncclCommInitAll over the
// distinct devices, root = the loaded model's device); replicas on a device that already holds
// a filled arena take a device-to-device copy.  librccl is opened on first use (dlopen), so the
// engine carries no link-time RCCL dependency.
namespace {
struct Rccl {
    decltype(&ncclCommInitAll) init = nullptr;
    decltype(&ncclBroadcast) bcast = nullptr;
    decltype(&ncclGroupStart) gstart = nullptr;
    decltype(&ncclGroupEnd) gend = nullptr;
    decltype(&ncclCommDestroy) destroy = nullptr;
    decltype(&ncclGetErrorString) err = nullptr;
    std::string load_error;     // why the library or a symbol is missing (dlerror() read once, here)
};
const Rccl& rccl() {
    static const Rccl r = [] {
        Rccl x;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) {
            const char* e = dlerror();
            x.load_error = e ? e : "dlopen(librccl.so) failed";
            return x;
        }
        x.init = reinterpret_cast<decltype(x.init)>(dlsym(h, "ncclCommInitAll"));
        x.bcast = reinterpret_cast<decltype(x.bcast)>(dlsym(h, "ncclBroadcast"));
        x.gstart = reinterpret_cast<decltype(x.gstart)>(dlsym(h, "ncclGroupStart"));
        x.gend = reinterpret_cast<decltype(x.gend)>(dlsym(h, "ncclGroupEnd"));
        x.destroy = reinterpret_cast<decltype(x.destroy)>(dlsym(h, "ncclCommDestroy"));
        x.err = reinterpret_cast<decltype(x.err)>(dlsym(h, "ncclGetErrorString"));
        if (!x.init || !x.bcast || !x.gstart || !x.gend || !x.destroy) x.load_error = "missing symbols";
        return x;
    }();
    return r;
}
// Diagnostic (MI_SEGV_MAPS=1): on SIGSEGV / SIGBUS print the fault address, the faulting PC and
// every backtrace frame with the mapping that holds it (path + offset, from /proc/self/maps), so
// the frames of a crash inside the ROCm libraries can be symbolised offline (llvm-symbolizer
// --obj=<path> <offset>); then the default action.  Installed when a context is created, i.e.
// after any profiler's own handler.
char g_maps[1 << 20];
void segv_out(const char* s) { ssize_t r = write(2, s, strlen(s)); (void)r; }
void segv_where(const char* tag, unsigned long long a, int nmaps) {
    char line[512];
    const char* p = g_maps;
    const char* end = g_maps + nmaps;
    const char* prev = nullptr;
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', end - p);
        if (!nl) nl = end;
        unsigned long long lo = 0, hi = 0, off = 0;
        if (sscanf(p, "%llx-%llx %*s %llx", &lo, &hi, &off) == 3 && a >= lo && a < hi) {
            const char* path = (const char*)memchr(p, '/', nl - p);
            const int pl = path ? (int)(nl - path) : 0;
            snprintf(line, sizeof line, "mi_segv %s 0x%llx = %.*s +0x%llx (mapping %.*s)\n", tag, a, pl, path ? path : "",
                     a - lo + off, (int)(nl - p), p);
            segv_out(line);
            return;
        }
        if (lo > a && prev) {   // unmapped: the mappings on either side
            const char* pn = (const char*)memchr(prev, '\n', end - prev);
            snprintf(line, sizeof line, "mi_segv %s 0x%llx unmapped, between\n  %.*s\n  %.*s\n", tag, a,
                     (int)((pn ? pn : end) - prev), prev, (int)(nl - p), p);
            segv_out(line);
            return;
        }
        prev = p;
        p = nl + 1;
    }
    snprintf(line, sizeof line, "mi_segv %s 0x%llx not found in maps\n", tag, a);
    segv_out(line);
}
void segv_handler(int sig, siginfo_t* si, void* ucv) {
    int fd = open("/proc/self/maps", O_RDONLY);
    int n = 0;
    if (fd >= 0) {
        for (ssize_t r; n < (int)sizeof(g_maps) - 1 && (r = read(fd, g_maps + n, sizeof(g_maps) - 1 - n)) > 0;) n += (int)r;
        close(fd);
    }
    char line[128];
    snprintf(line, sizeof line, "mi_segv signal %d fault address %p\n", sig, si ? si->si_addr : nullptr);
    segv_out(line);
    segv_where("fault", (unsigned long long)(si ? si->si_addr : nullptr), n);
    const ucontext_t* uc = reinterpret_cast<const ucontext_t*>(ucv);
    if (uc) segv_where("pc", (unsigned long long)uc->uc_mcontext.gregs[REG_RIP], n);
    void* fr[64];
    const int nf = backtrace(fr, 64);
    for (int i = 0; i < nf; ++i) {
        char tag[16];
        snprintf(tag, sizeof tag, "frame%02d", i);
        segv_where(tag, (unsigned long long)fr[i], n);
    }
    signal(sig, SIG_DFL);
    raise(sig);
}
void segv_maps_install() {
    static bool done = false;
    if (done || !getenv("MI_SEGV_MAPS")) return;
    done = true;
    void* warm[2];
    backtrace(warm, 2);   // loads the unwinder before any signal
    struct sigaction sa;
    memset(&sa, 0, sizeof sa);
    sa.sa_sigaction = segv_handler;
    sa.sa_flags = SA_SIGINFO;
    sigaction(SIGSEGV, &sa, nullptr);
    sigaction(SIGBUS, &sa, nullptr);
    segv_out("mi_segv: handler installed\n");
}
void nccl_ck(ncclResult_t r, const char* what) {
    if (r != ncclSuccess) throw Error(std::string("RCCL ") + what + ": " + (rccl().err ? rccl().err(r) : "error"));
}
}  // namespace

extern "C" {

const char* mi_last_error(void) { return last_error(); }

mi_model* mi_model_load_from_memory(const void* data, size_t size, const mi_model_params* params) {
    try {
        set_last_error("");
        mi_model_params p{0, 0, 0, 0};
        if (params) p = *params;
        if (p.cpu_only) throw Error("cpu_only: the CPU path is the reference's ggml backend, not this engine");
        auto* m = new mi_model();
        try {
            m->impl.load(static_cast<const uint8_t*>(data), size, p);
        } catch (...) {
            delete m;
            throw;
        }
        return m;
    }
    MI_TRY(nullptr)
}

mi_model* mi_model_load(const char* path, const mi_model_params* params) {
    try {
        if (!path) throw Error("null path");
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) throw Error(std::string("cannot open ") + path);
        struct stat st;
        if (fstat(fd, &st) != 0) { ::close(fd); throw Error("fstat failed"); }
        const size_t size = (size_t)st.st_size;
        void* map = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        ::close(fd);
        if (map == MAP_FAILED) throw Error(std::string("mmap failed for ") + path);
        mi_model* m = mi_model_load_from_memory(map, size, params);
        munmap(map, size);
        return m;
    }
    MI_TRY(nullptr)
}

void mi_model_free(mi_model* model) { delete model; }

int32_t mi_model_n_vocab(const mi_model* m) { return m ? m->impl.hp.n_vocab : -1; }
int32_t mi_model_n_ctx_train(const mi_model* m) { return m ? m->impl.hp.n_ctx_train : -1; }
int32_t mi_model_n_embd(const mi_model* m) { return m ? m->impl.hp.n_embd : -1; }
int32_t mi_model_n_layer(const mi_model* m) { return m ? m->impl.hp.n_layer : -1; }
int32_t mi_model_n_head(const mi_model* m) { return m ? m->impl.hp.n_head : -1; }
int32_t mi_model_n_head_kv(const mi_model* m) { return m ? m->impl.hp.n_head_kv : -1; }
int32_t mi_model_n_ff(const mi_model* m) { return m ? m->impl.hp.n_ff : -1; }
int32_t mi_model_n_expert(const mi_model* m) { return m ? m->impl.hp.n_expert : -1; }
float mi_model_rope_freq_scale(const mi_model* m) { return m ? m->impl.hp.freq_scale : 0.0f; }
int32_t mi_model_token_bos(const mi_model* m) { return m ? m->impl.bos : -1; }
int32_t mi_model_token_eos(const mi_model* m) { return m ? m->impl.eos : -1; }
int32_t mi_model_add_bos(const mi_model* m) { return m ? (m->impl.add_bos ? 1 : 0) : -1; }

int32_t mi_model_token_is_eog(const mi_model* m, int32_t token) {
    if (!m) return -1;
    return (token == m->impl.eos || (m->impl.eot >= 0 && token == m->impl.eot)) ? 1 : 0;
}

float mi_model_token_score(const mi_model* m, int32_t token) {
    if (!m || token < 0 || token >= (int)m->impl.token_score.size()) return 0.0f;
    return m->impl.token_score[token];
}

int32_t mi_model_token_type(const mi_model* m, int32_t token) {
    if (!m || token < 0 || token >= (int)m->impl.tokens.size()) return -1;
    if (token >= (int)m->impl.token_type.size()) return 1;   // LLAMA_TOKEN_TYPE_NORMAL
    return m->impl.token_type[token];
}

int32_t mi_model_n_tokens(const mi_model* m) { return m ? (int32_t)m->impl.tokens.size() : -1; }

int32_t mi_model_tokenizer(const mi_model* m, char* buf, int32_t size) {
    if (!m) return -1;
    const std::string& s = m->impl.tok_model;
    if (buf && size > 0) {
        const int n = std::min<int>((int)s.size(), size - 1);
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return (int32_t)s.size();
}

int32_t mi_model_token_text(const mi_model* m, int32_t token, char* buf, int32_t size) {
    if (!m || token < 0 || token >= (int)m->impl.tokens.size()) { set_last_error("token out of range"); return -1; }
    const std::string& s = m->impl.tokens[token];
    if (buf && size > 0) {
        const int n = std::min<int>((int)s.size(), size - 1);
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return (int32_t)s.size();
}

int32_t mi_model_n_merges(const mi_model* m) { return m ? (int32_t)m->impl.merges.size() : -1; }

int32_t mi_model_merge(const mi_model* m, int32_t i, char* buf, int32_t size) {
    if (!m || i < 0 || i >= (int)m->impl.merges.size()) { set_last_error("merge out of range"); return -1; }
    const std::string& s = m->impl.merges[i];
    if (buf && size > 0) {
        const int n = std::min<int>((int)s.size(), size - 1);
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return (int32_t)s.size();
}

int32_t mi_model_meta_str(const mi_model* m, const char* key, char* buf, int32_t size) {
    if (!m || !key) return -1;
    const GgufValue* v = m->impl.gguf.get(key);
    if (!v) return -1;
    std::string s = v->type == 8 ? v->s : (v->type == 6 || v->type == 12) ? std::to_string(v->f) : std::to_string(v->i);
    if (buf && size > 0) {
        const int n = std::min<int>((int)s.size(), size - 1);
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return (int32_t)s.size();
}

int64_t mi_model_weight_bytes(const mi_model* m) { return m ? m->impl.weight_bytes : -1; }

int32_t mi_model_arena(const mi_model* m, void** dev_ptr, size_t* bytes) {
    if (!m) return -1;
    if (dev_ptr) *dev_ptr = m->impl.arena;
    if (bytes) *bytes = m->impl.arena_bytes;
    return 0;
}


// One line per replication stage on stderr: a start-up that dies inside RCCL or HIP says where.
static void replicate_log(const std::string& what) {
    std::fprintf(stderr, "mi_engine: replicate: %s\n", what.c_str());
    std::fflush(stderr);
}

int32_t mi_model_replicate(mi_model* const* models, int32_t n) {
    int caller_dev = -1;
    (void)hipGetDevice(&caller_dev);
    // communicators and streams are released on every path (a throw after ncclCommInitAll included)
    struct Guard {
        std::vector<ncclComm_t> comms;
        std::vector<std::pair<int, hipStream_t>> streams;
        int dev;
        ~Guard() {
            for (auto& [d, s] : streams) {
                if (!s) continue;
                (void)hipSetDevice(d);
                (void)hipStreamSynchronize(s);
                (void)hipStreamDestroy(s);
            }
            for (ncclComm_t c : comms)
                if (c && rccl().destroy) rccl().destroy(c);
            if (dev >= 0) (void)hipSetDevice(dev);
        }
    } guard{{}, {}, caller_dev};
    try {
        if (!models || n < 1 || !models[0]) throw Error("replicate: no source model");
        const Model& src = models[0]->impl;
        if (!src.arena) throw Error("replicate: the source model has no weights");
        for (int i = 1; i < n; ++i) {
            const Model& d = models[i]->impl;
            if (!d.arena || d.arena_bytes != src.arena_bytes || d.gguf.tensors.size() != src.gguf.tensors.size())
                throw Error("replicate: replica " + std::to_string(i) + " was not loaded from the same GGUF header");
            // the MFMA-order copies are built from the arena when the first context needs them
            if (d.mmq_arena) throw Error("replicate: replica " + std::to_string(i) + " already has a context");
        }
        std::vector<int> filled(n, 0);
        filled[0] = 1;
        // one receiver per distinct device other than the source's (RCCL ranks 1..); MI_REPLICATE_RCCL=1
        // also sends the first same-device replica through a one-rank broadcast (exercises the path on
        // a single GPU)
        std::vector<int> devs = {src.device}, recv = {0};
        const bool force = getenv("MI_REPLICATE_RCCL") != nullptr;
        for (int i = 1; i < n; ++i) {
            const int dv = models[i]->impl.device;
            if (std::find(devs.begin(), devs.end(), dv) == devs.end()) {
                devs.push_back(dv);
                recv.push_back(i);
            }
        }
        int self_recv = -1;
        if (force && devs.size() == 1)
            for (int i = 1; i < n && self_recv < 0; ++i)
                if (models[i]->impl.device == src.device) self_recv = i;
        replicate_log(std::to_string(n) + " models, " + std::to_string(src.arena_bytes) + " B arena, " +
                      std::to_string(devs.size()) + " device(s)" + (self_recv > 0 ? ", one-rank RCCL broadcast forced" : ""));
        if (devs.size() > 1 || self_recv > 0) {
            const Rccl& R = rccl();
            if (!R.init || !R.bcast || !R.gstart || !R.gend || !R.destroy)
                throw Error("replicate: librccl not usable: " + R.load_error);
            const int nd = (int)devs.size();
            guard.comms.assign(nd, nullptr);
            replicate_log("ncclCommInitAll over " + std::to_string(nd) + " device(s)");
            nccl_ck(R.init(guard.comms.data(), nd, devs.data()), "ncclCommInitAll");
            replicate_log("communicators ready");
            for (int r = 0; r < nd; ++r) {
                MI_HIP(hipSetDevice(devs[r]));
                hipStream_t s = nullptr;
                MI_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
                guard.streams.emplace_back(devs[r], s);
            }
            replicate_log("ncclBroadcast of the arena");
            nccl_ck(R.gstart(), "ncclGroupStart");
            for (int r = 0; r < nd; ++r) {
                MI_HIP(hipSetDevice(devs[r]));
                uint8_t* dst = r == 0 ? (self_recv > 0 ? models[self_recv]->impl.arena : src.arena)
                                      : models[recv[r]]->impl.arena;
                nccl_ck(R.bcast(src.arena, dst, src.arena_bytes, ncclUint8, 0, guard.comms[r], guard.streams[r].second),
                        "ncclBroadcast");
            }
            nccl_ck(R.gend(), "ncclGroupEnd");
            for (auto& [d, s] : guard.streams) {
                MI_HIP(hipSetDevice(d));
                MI_HIP(hipStreamSynchronize(s));
            }
            replicate_log("broadcast complete");
            for (int r = 1; r < nd; ++r) filled[recv[r]] = 1;
            if (self_recv > 0) filled[self_recv] = 1;
        }
        // the rest: a copy from a filled arena on the same device (or a peer copy from the source)
        for (int i = 1; i < n; ++i) {
            if (filled[i]) continue;
            Model& d = models[i]->impl;
            const uint8_t* from = src.arena;
            int from_dev = src.device;
            for (int j = 0; j < n; ++j)
                if (filled[j] && models[j]->impl.device == d.device) { from = models[j]->impl.arena; from_dev = d.device; break; }
            replicate_log("replica " + std::to_string(i) + ": device copy " + std::to_string(from_dev) + " -> " +
                          std::to_string(d.device));
            MI_HIP(hipSetDevice(d.device));
            if (from_dev == d.device) MI_HIP(hipMemcpy(d.arena, from, src.arena_bytes, hipMemcpyDeviceToDevice));
            else MI_HIP(hipMemcpyPeer(d.arena, d.device, from, from_dev, src.arena_bytes));
            filled[i] = 1;
        }
        for (int i = 0; i < n; ++i) {
            MI_HIP(hipSetDevice(models[i]->impl.device));
            MI_HIP(hipDeviceSynchronize());
        }
        replicate_log("done");
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_model_type_histogram(const mi_model* m, int64_t* out, int32_t n) {
    if (!m || !out) return -1;
    const int k = std::min(n, 32);
    for (int i = 0; i < k; ++i) out[i] = m->impl.type_bytes[i];
    return k;
}

mi_ctx* mi_ctx_create(mi_model* model, uint32_t n_ctx, uint32_t n_batch, uint32_t n_ubatch) {
    try {
        if (!model) throw Error("null model");
        segv_maps_install();
        auto* c = new mi_ctx();
        try {
            c->impl.reset(new Ctx(&model->impl, n_ctx, n_batch, n_ubatch));
        } catch (...) {
            delete c;
            throw;
        }
        return c;
    }
    MI_TRY(nullptr)
}

void mi_ctx_free(mi_ctx* ctx) { delete ctx; }
uint32_t mi_n_ctx(const mi_ctx* c) { return c ? c->impl->n_ctx : 0; }
uint32_t mi_n_batch(const mi_ctx* c) { return c ? c->impl->n_batch : 0; }

int32_t mi_decode(mi_ctx* c, const int32_t* tokens, int32_t n, int32_t out_mode) {
    try {
        if (!c || !tokens) throw Error("null argument");
        if (out_mode != MI_OUT_LAST && out_mode != MI_OUT_ALL) throw Error("decode: out_mode must be MI_OUT_LAST or MI_OUT_ALL");
        return c->impl->decode(tokens, n, out_mode == MI_OUT_ALL);
    }
    MI_TRY(-1)
}

int32_t mi_topk(mi_ctx* c, int32_t row, int32_t k, int32_t* ids, float* logits) {
    try {
        if (!c || !ids || !logits) throw Error("null argument");
        return c->impl->topk(row, k, ids, logits);
    }
    MI_TRY(-1)
}

int32_t mi_gather(mi_ctx* c, int32_t row, const int32_t* ids, int32_t n, float* out) {
    try {
        if (!c || (n > 0 && (!ids || !out))) throw Error("null argument");
        return c->impl->gather(row, ids, n, out);
    }
    MI_TRY(-1)
}

int32_t mi_gather_rows(mi_ctx* c, int32_t row0, int32_t n_rows, const int32_t* ids, int32_t k, float* out) {
    try {
        if (!c || ((int64_t)n_rows * k > 0 && (!ids || !out))) throw Error("null argument");
        return c->impl->gather_rows(row0, n_rows, ids, k, out);
    }
    MI_TRY(-1)
}

const float* mi_logits(mi_ctx* c, int32_t row) {
    try {
        if (!c) throw Error("null ctx");
        return c->impl->logits_host(row);
    }
    MI_TRY(nullptr)
}

void mi_synchronize(mi_ctx* c) {
    try { if (c) c->impl->sync(); } catch (const std::exception& e) { set_last_error(e.what()); }
}

void mi_kv_clear(mi_ctx* c) { if (c) c->impl->kv_clear(); }

int32_t mi_kv_seq_rm(mi_ctx* c, int32_t p0, int32_t p1) {
    try { if (!c) throw Error("null ctx"); return c->impl->kv_seq_rm(p0, p1); }
    MI_TRY(-1)
}
int32_t mi_kv_seq_add(mi_ctx* c, int32_t p0, int32_t p1, int32_t delta) {
    try { if (!c) throw Error("null ctx"); return c->impl->kv_seq_shift(p0, p1, delta, 0); }
    MI_TRY(-1)
}
int32_t mi_kv_seq_div(mi_ctx* c, int32_t p0, int32_t p1, int32_t d) {
    try {
        if (!c) throw Error("null ctx");
        if (d <= 0) throw Error("seq_div: divisor must be positive");
        return c->impl->kv_seq_shift(p0, p1, 0, d);
    }
    MI_TRY(-1)
}
int32_t mi_kv_pos_max(const mi_ctx* c) { return c ? c->impl->pos_max : -1; }
int32_t mi_kv_n_cells(const mi_ctx* c) { return c ? c->impl->n_cells : -1; }

size_t mi_state_size(mi_ctx* c) { return c ? c->impl->state_size() : 0; }
size_t mi_state_get(mi_ctx* c, uint8_t* dst, size_t size) {
    try { if (!c || !dst) throw Error("null argument"); return c->impl->state_get(dst, size); }
    MI_TRY(0)
}
size_t mi_state_set(mi_ctx* c, const uint8_t* src, size_t size) {
    try { if (!c || !src) throw Error("null argument"); return c->impl->state_set(src, size); }
    MI_TRY(0)
}

int32_t mi_ctx_apply_cvec(mi_ctx* c, const float* data, size_t len, int32_t n_embd, int32_t il_start, int32_t il_end) {
    try {
        if (!c) throw Error("null ctx");
        c->impl->apply_cvec(data, len, n_embd, il_start, il_end);
        return 0;
    }
    MI_TRY(-1)
}

// The loader of one control-vector GGUF: every tensor must be an F32, 1-D "direction.N" (N >= 1),
// all of one length; data[n_embd * (N - 1) + j] += src[j] * strength.
int64_t mi_cvec_load(const char* path, float strength, float* data, size_t cap, int32_t* n_embd_out) {
    try {
        if (!path) throw Error("null path");
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) throw Error(std::string("cannot open ") + path);
        struct stat st;
        if (fstat(fd, &st) != 0) { ::close(fd); throw Error("fstat failed"); }
        const size_t size = (size_t)st.st_size;
        std::vector<uint8_t> img(size);
        size_t got = 0;
        while (got < size) {
            const ssize_t r = ::read(fd, img.data() + got, size - got);
            if (r <= 0) break;
            got += (size_t)r;
        }
        ::close(fd);
        if (got != size) throw Error(std::string("cannot read ") + path);
        Gguf g;
        g.parse(img.data(), size);
        long long n_embd = -1, max_n = 0;
        std::vector<long long> layer(g.tensors.size());
        for (size_t i = 0; i < g.tensors.size(); ++i) {
            const GgufTensor& t = g.tensors[i];
            long long n = -1;
            if (t.name.compare(0, 10, "direction.") == 0 && t.name.size() > 10 && t.name.size() <= 19) {
                // (std::stoi's reading: optional sign, digits, anything after them ignored)
                const char* s = t.name.c_str() + 10;
                char* end = nullptr;
                const long long v = std::strtoll(s, &end, 10);
                if (end != s) n = v;
            }
            if (n <= 0) throw Error("control vector: tensor '" + t.name + "' is not direction.N with N >= 1");
            if (t.type != T_F32) throw Error("control vector: " + t.name + " is not F32");
            if (t.n_dims != 1) throw Error("control vector: " + t.name + " is not 1-D");
            if (n_embd < 0) n_embd = t.ne[0];
            else if (t.ne[0] != n_embd) throw Error("control vector: " + t.name + " differs in length from the others");
            if (g.data_offset + t.offset + (size_t)t.ne[0] * 4 > size) throw Error("control vector: tensor data beyond the end of the file");
            layer[i] = n;
            max_n = std::max(max_n, n);
        }
        if (n_embd <= 0 || n_embd > INT32_MAX) throw Error("control vector: no direction tensors");
        if (n_embd_out) *n_embd_out = (int32_t)n_embd;
        const long long need = n_embd * max_n;
        if (data && cap >= (size_t)need) {
            for (size_t i = 0; i < g.tensors.size(); ++i) {
                const uint8_t* src = img.data() + g.data_offset + g.tensors[i].offset;
                float* dst = data + n_embd * (layer[i] - 1);
                for (long long j = 0; j < n_embd; ++j) {
                    float v;
                    std::memcpy(&v, src + 4 * j, 4);
                    dst[j] += v * strength;
                }
            }
        }
        return need;
    }
    MI_TRY(-1)
}

// ---- LoRA adapters (lora.cpp) ----
mi_lora* mi_lora_load_from_memory(mi_model* model, const void* data, size_t size) {
    try {
        set_last_error("");
        if (!model) throw Error("null model");
        if (!data) throw Error("null adapter image");
        std::unique_ptr<mi_lora> a(new mi_lora());
        a->impl = Lora::load(&model->impl, static_cast<const uint8_t*>(data), size);
        return a.release();
    }
    MI_TRY(nullptr)
}

mi_lora* mi_lora_load(mi_model* model, const char* path) {
    try {
        if (!path) throw Error("null path");
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) throw Error(std::string("cannot open ") + path);
        struct stat st;
        if (fstat(fd, &st) != 0) { ::close(fd); throw Error("fstat failed"); }
        const size_t size = (size_t)st.st_size;
        if (size == 0) { ::close(fd); throw Error(std::string("empty file ") + path); }
        void* map = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        ::close(fd);
        if (map == MAP_FAILED) throw Error(std::string("mmap failed for ") + path);
        mi_lora* a = mi_lora_load_from_memory(model, map, size);
        munmap(map, size);
        return a;
    }
    MI_TRY(nullptr)
}

void mi_lora_free(mi_lora* a) { delete a; }
float mi_lora_alpha(const mi_lora* a) { return a ? a->impl->alpha : 0.0f; }
int32_t mi_lora_n_pairs(const mi_lora* a) { return a ? (int32_t)a->impl->pairs.size() : -1; }

int32_t mi_ctx_set_lora(mi_ctx* c, mi_lora* a, float scale) {
    try {
        if (!c) throw Error("null ctx");
        if (!a) throw Error("null adapter");
        c->impl->set_lora(a->impl, scale);
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_ctx_rm_lora(mi_ctx* c, mi_lora* a) {
    try {
        if (!c) throw Error("null ctx");
        if (!a) throw Error("null adapter");
        if (a->impl->m != c->impl->m) throw Error("rm_lora: the adapter belongs to another model");
        if (c->impl->rm_lora(a->impl.get()) != 0) throw Error("rm_lora: the adapter is not set on this context");
        return 0;
    }
    MI_TRY(-1)
}

void mi_ctx_clear_lora(mi_ctx* c) {
    try { if (c) c->impl->clear_lora(); } catch (const std::exception& e) { set_last_error(e.what()); }
}

// ---- embeddings ----
int32_t mi_model_pooling_type(const mi_model* m) { return m ? m->impl.hp.pooling_type : -1; }
int32_t mi_model_causal_attn(const mi_model* m) { return m ? (m->impl.hp.arch == ARCH_BERT ? 0 : 1) : -1; }

int32_t mi_ctx_set_embeddings(mi_ctx* c, int32_t on, int32_t pooling) {
    try {
        if (!c) throw Error("null ctx");
        c->impl->set_embeddings(on != 0, pooling);
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_ctx_pooling(const mi_ctx* c) { return c ? c->impl->pooling : -1; }

const float* mi_embeddings(mi_ctx* c, int32_t row) {
    try {
        if (!c) throw Error("null ctx");
        return c->impl->embeddings_host(row);
    }
    MI_TRY(nullptr)
}

int32_t mi_prof_enable(mi_ctx* c, int32_t layer) {
    if (!c) return -1;
    if (layer >= c->impl->m->hp.n_layer) layer = c->impl->m->hp.n_layer - 1;
    if (c->impl->prof_layer != layer) {
        c->impl->prof_layer = layer < 0 ? -1 : layer;
        c->impl->invalidate_graphs();
    }
    return 0;
}
int32_t mi_prof_read(mi_ctx* c, float* us, int32_t n) {
    try { if (!c || !us) throw Error("null argument"); return c->impl->prof_read(us, n); }
    MI_TRY(-1)
}
int64_t mi_prof_ffn_bytes(const mi_ctx* c) { return c ? c->impl->ffn_bytes() : -1; }
int64_t mi_prof_bytes(const mi_ctx* c) { return c ? c->impl->prof_bytes : -1; }

int32_t mi_decode_path(const mi_ctx* c) {
    if (!c) return -1;
    if (c->impl->enc) return 2;
    if (c->impl->m->f16) return 3;
    return c->impl->sp_ok ? 1 : 0;
}
int32_t mi_batch_path(const mi_ctx* c) { return c ? c->impl->batch_path : -1; }
int32_t mi_debug_stamps(mi_ctx* c, uint64_t* out, int32_t n_launch) {
    try {
        if (!c || !out) throw Error("null argument");
        mi::Ctx* x = c->impl.get();
        if (!x->stamps) return 0;
        n_launch = std::min(n_launch, (int32_t)mi::Ctx::kStampLaunches);
        x->sync();
        MI_HIP(hipMemcpy(out, x->stamps, (size_t)n_launch * mi::Ctx::kStampWgs * 8 * 8, hipMemcpyDeviceToHost));
        return n_launch;
    }
    MI_TRY(-1)
}
int32_t mi_debug_down_quant(mi_ctx* c, int32_t form) {
    try {
        if (!c) throw Error("null argument");
        c->impl->set_down_quant(form);
        return 0;
    }
    MI_TRY(-1)
}

}  // extern "C"
