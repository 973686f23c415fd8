// rf_api_take.hip -- rf_corpus_take / rf_corpus_take_u32 / rf_corpus_lengths / rf_corpus_is_wide: the candidates behind the indices every result road returns,
// read back out of the packed corpus (kernels: rf_take.hip), and rf_host_layout_candidate, the same inverse over a host layout without a device.  Both sides
// address the payload through rf_take_addr.hpp.  Product code: never includes or links anything from oracle/.
#include "rf_host.hpp"

#include "rf_take_addr.hpp"

extern "C" {

rf_status rf_host_layout_candidate(const rf_host_layout* l, uint64_t index, uint8_t* out, uint64_t capacity, uint32_t* out_len)
try {
    if (!l || !out_len || (capacity && !out) || index >= l->n) {
        set_error("rf_host_layout_candidate: null argument or index beyond the layout's candidates");
        return RF_ERR_INVALID_ARG;
    }
    uint64_t slot = index;
    if (!l->identity) {
        slot = l->n_slots;
        for (uint64_t s = 0; s < l->n_slots; ++s)
            if (l->orig[s] == index) {
                slot = s;
                break;
            }
    }
    const uint32_t t = take_tile_of(slot), lane = take_lane_of(slot);
    if (slot >= (uint64_t)l->n_tiles * kTakeLanes) {
        set_error("rf_host_layout_candidate: the layout names no slot for this candidate");
        return RF_ERR_INVALID_ARG;
    }
    // (an identity layout has descriptors too: tile t at t * take_tile_bytes(len), which is what take_uniform_base says)
    const uint32_t len = l->tile_len[t];
    const uint64_t base = l->identity ? take_uniform_base(t, len) : l->tile_off[t];
    uint8_t inv[256];
    take_inverse_sigma(l->sigma, inv);
    const uint64_t take = std::min<uint64_t>(len, capacity);
    for (uint64_t b = 0; b < take; ++b) out[b] = inv[l->packed[take_byte_at(base, lane, (uint32_t)b)]];
    *out_len = len;
    return RF_OK;
}
RF_ABI_CATCH

int rf_corpus_is_wide(const rf_corpus* c) { return c && c->wide ? 1 : 0; }

// candidate -> slot of a length-bucketed corpus, built on first use under rf_corpus::Accel's rule (local owner, synchronize, then move under scratch_mu); the
// gather path's copy serves when it is there.  The address never changes once handed out: the buffer only ever moves between the two owners.
rf_status corpus_take_slot_of(const rf_corpus* c, hipStream_t st, const uint32_t** out)
{
    std::lock_guard<std::mutex> lock(c->scratch_mu);
    rf_corpus::Accel& a = c->accel;
    if (!a.gather.slot_of.ptr && !a.take_slot_of.ptr) {
        DeviceBuf local;
        RF_HIP(local.reserve(c->n * sizeof(uint32_t)));
        RF_HIP(hipMemsetAsync(local.ptr, 0xFF, c->n * sizeof(uint32_t), st));  // (a slot map that names no slot for a candidate: the kernels read it as empty)
        RF_HIP(launch_slot_maps(c->d_orig, (uint32_t)c->n_slots, local.as<uint32_t>(), nullptr, st));
        RF_HIP(hipStreamSynchronize(st));
        a.take_slot_of = std::move(local);
    }
    *out = a.gather.slot_of.ptr ? a.gather.slot_of.as<uint32_t>() : a.take_slot_of.as<uint32_t>();
    return RF_OK;
}

namespace {
// the host arrays a call enqueues copies from or to stay alive until the stream has drained, on every way out
struct StreamDrain {
    hipStream_t st;
    ~StreamDrain() { (void)hipStreamSynchronize(st); }
};

struct TakeCall {
    const char* who;
    const rf_corpus* c;
    const uint64_t* indices;
    size_t m;
    uint64_t index_base;
};

// the checks rf_corpus_take* and rf_corpus_lengths share: nothing of a device, nothing written
rf_status take_check(const TakeCall& k, const void* out_meta)
{
    auto bad = [&](const char* why) {
        set_error(std::string(k.who) + ": " + why);
        return RF_ERR_INVALID_ARG;
    };
    if (!k.c) return bad("null corpus");
    if (!out_meta) return bad("null output");
    if (k.c->borrowed) return bad("not a packed corpus");
    if (!k.indices) return k.m == k.c->n ? RF_OK : bad("indices == NULL asks for every candidate: m must be rf_corpus_count");
    for (size_t j = 0; j < k.m; ++j)
        if (k.indices[j] < k.index_base || k.indices[j] - k.index_base >= k.c->n) return bad("an index lies outside [index_base, index_base + n)");
    return RF_OK;
}

// the part of TakeParams that is the corpus; `tables` (device, 1280 bytes) receives the id -> symbol table and the inverse renaming from `host_tables`
rf_status take_corpus_params(const rf_corpus* c, bool symbols, uint8_t* tables, uint32_t* host_tables, hipStream_t st, TakeParams* p)
{
    *p = TakeParams{};
    p->s.data = c->d_data;
    p->s.tiles = c->uniform ? nullptr : c->d_tiles;
    p->s.orig = c->uniform ? nullptr : c->d_orig;
    p->s.n = (uint32_t)c->n;
    p->s.n_tiles = c->n_tiles;
    p->s.uniform_len = c->uniform_len;
    p->s.uniform_tile_bytes = (uint32_t)tile_bytes(c->uniform_len);
    p->n_slots = c->uniform ? c->n_tiles * (uint32_t)kWave : (uint32_t)c->n_slots;
    if (!symbols) return RF_OK;
    for (uint32_t id = 0; id < 256; ++id) host_tables[id] = c->wide ? 0xFFFFFFFFu : id;  // (an id no symbol has is never stored)
    for (const auto& kv : c->alphabet) host_tables[kv.second] = kv.first;
    take_inverse_sigma(c->sigma, reinterpret_cast<uint8_t*>(host_tables + 256));
    RF_HIP(hipMemcpyAsync(tables, host_tables, 1280, hipMemcpyHostToDevice, st));
    p->sym_of_id = c->wide ? reinterpret_cast<const uint32_t*>(tables) : nullptr;
    p->inv_sigma = tables + 1024;
    p->raw = c->d_raw;
    p->raw_elem = c->raw_elem;
    return RF_OK;
}

// row_len (device) of the requested rows / of every candidate: take_rows_len_kernel, or -- every candidate of a length-bucketed corpus -- one pass over the tiles
rf_status take_lengths_device(const TakeCall& k, TakeParams& p, ScratchSet& scratch, const std::vector<uint32_t>& idx, hipStream_t st)
{
    const rf_corpus* c = k.c;
    RF_HIP(scratch.get(&p.row_len, k.m * sizeof(uint32_t)));
    if (!k.indices) {
        RF_HIP(hipMemsetAsync(p.row_len, 0, k.m * sizeof(uint32_t), st));  // (a candidate no slot names reads as empty)
        RF_HIP(launch_len_of(c->d_tiles, c->n_tiles, c->d_orig, p.row_len, st));
        return RF_OK;
    }
    uint32_t* d_idx = nullptr;
    RF_HIP(scratch.get(&d_idx, k.m * sizeof(uint32_t)));
    RF_HIP(scratch.get(&p.row_slot, k.m * sizeof(uint32_t)));
    RF_HIP(hipMemcpyAsync(d_idx, idx.data(), k.m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    p.idx = d_idx;
    p.m = k.m;
    if (!c->uniform) {
        const rf_status s = corpus_take_slot_of(c, st, &p.slot_of);
        if (s != RF_OK) return s;
    }
    RF_HIP(launch_take_rows_len(p, st));
    return RF_OK;
}

std::vector<uint32_t> local_indices(const TakeCall& k)
{
    std::vector<uint32_t> idx(k.indices ? k.m : 0);
    for (size_t j = 0; j < idx.size(); ++j) idx[j] = (uint32_t)(k.indices[j] - k.index_base);
    return idx;
}

rf_status take_impl(const TakeCall& k, bool out_u32, void* out, uint64_t capacity, uint64_t* out_offsets, rf_mem out_mem, void* stream)
{
    rf_status s = take_check(k, out_offsets);
    if (s != RF_OK) return s;
    const rf_corpus* c = k.c;
    if ((out_mem != RF_MEM_HOST && out_mem != RF_MEM_DEVICE) || (capacity && !out) || (!out_u32 && c->wide)) {
        set_error(std::string(k.who) + (!out_u32 && c->wide ? ": a corpus packed by rf_corpus_pack_u32 is read with rf_corpus_take_u32" : ": unknown out_mem, or a null payload with a capacity"));
        return RF_ERR_INVALID_ARG;
    }
    out_offsets[0] = 0;
    if (k.m == 0) return RF_OK;
    const size_t m = k.m, elem = out_u32 ? sizeof(uint32_t) : 1;
    const bool all_uniform = !k.indices && c->uniform;  // every candidate of a single-length corpus: the offsets are arithmetic
    DeviceGuard guard(c->device);
    if (!guard.ok) {
        set_error("cannot select the corpus' device");
        return RF_ERR_NO_DEVICE;
    }
    hipStream_t st = (hipStream_t)stream;
    std::vector<uint32_t> idx = local_indices(k), lens;
    uint32_t host_tables[320];
    ScratchSet scratch(st);
    StreamDrain drain{st};
    uint8_t* d_tables = nullptr;
    RF_HIP(scratch.get(&d_tables, 1280));
    TakeParams p;
    if ((s = take_corpus_params(c, true, d_tables, host_tables, st, &p)) != RF_OK) return s;
    p.out_u32 = out_u32 ? 1u : 0u;
    // ---- lengths -> offsets, on the host (the total comes home anyway)
    uint32_t longest = 0;
    if (all_uniform) {
        for (size_t j = 0; j < m; ++j) out_offsets[j + 1] = (uint64_t)(j + 1) * c->uniform_len;
        longest = c->uniform_len;
    } else {
        if ((s = take_lengths_device(k, p, scratch, idx, st)) != RF_OK) return s;
        lens.resize(m);
        RF_HIP(copy_home(lens.data(), p.row_len, m * sizeof(uint32_t), st));
        for (size_t j = 0; j < m; ++j) {
            out_offsets[j + 1] = out_offsets[j] + lens[j];
            longest = std::max(longest, lens[j]);
        }
    }
    const uint64_t total = out_offsets[m];
    if (capacity == 0) return RF_OK;  // a sizing call
    if (capacity < total) {
        set_error(std::string(k.who) + ": capacity is smaller than the total the offsets report");
        return RF_ERR_INVALID_ARG;
    }
    if (total == 0) return RF_OK;
    // ---- the symbols
    void* dst = out;
    if (out_mem == RF_MEM_HOST) RF_HIP(scratch.get(reinterpret_cast<uint8_t**>(&dst), total * elem));
    p.out = dst;
    if (!all_uniform) {
        uint64_t* d_off = nullptr;
        RF_HIP(scratch.get(&d_off, m * sizeof(uint64_t)));
        RF_HIP(hipMemcpyAsync(d_off, out_offsets, m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        p.offsets = d_off;
    }
    p.row_chunks = take_chunks(longest);
    RF_HIP(k.indices ? launch_take_rows(p, st) : launch_take_all(p, st));
    if (out_mem == RF_MEM_HOST) RF_HIP(hipMemcpyAsync(out, dst, total * elem, hipMemcpyDeviceToHost, st));
    RF_HIP(hipStreamSynchronize(st));
    return RF_OK;
}
}  // namespace

rf_status rf_corpus_lengths(const rf_corpus* c, const uint64_t* indices, size_t m, uint64_t index_base, uint32_t* out_len, void* stream)
try {
    const TakeCall k{"rf_corpus_lengths", c, indices, m, index_base};
    rf_status s = take_check(k, out_len);
    if (s != RF_OK || m == 0) return s;
    if (c->uniform) {
        std::fill(out_len, out_len + m, c->uniform_len);
        return RF_OK;
    }
    DeviceGuard guard(c->device);
    if (!guard.ok) {
        set_error("cannot select the corpus' device");
        return RF_ERR_NO_DEVICE;
    }
    hipStream_t st = (hipStream_t)stream;
    std::vector<uint32_t> idx = local_indices(k);
    ScratchSet scratch(st);
    StreamDrain drain{st};
    TakeParams p;
    if ((s = take_corpus_params(c, false, nullptr, nullptr, st, &p)) != RF_OK) return s;
    if ((s = take_lengths_device(k, p, scratch, idx, st)) != RF_OK) return s;
    RF_HIP(copy_home(out_len, p.row_len, m * sizeof(uint32_t), st));
    return RF_OK;
}
RF_ABI_CATCH

rf_status rf_corpus_take(const rf_corpus* c, const uint64_t* indices, size_t m, uint64_t index_base, uint8_t* out_bytes, uint64_t capacity, uint64_t* out_offsets,
                         rf_mem out_mem, void* stream)
try {
    return take_impl(TakeCall{"rf_corpus_take", c, indices, m, index_base}, false, out_bytes, capacity, out_offsets, out_mem, stream);
}
RF_ABI_CATCH

rf_status rf_corpus_take_u32(const rf_corpus* c, const uint64_t* indices, size_t m, uint64_t index_base, uint32_t* out_elems, uint64_t capacity,
                             uint64_t* out_offsets, rf_mem out_mem, void* stream)
try {
    return take_impl(TakeCall{"rf_corpus_take_u32", c, indices, m, index_base}, true, out_elems, capacity, out_offsets, out_mem, stream);
}
RF_ABI_CATCH

}  // extern "C"
