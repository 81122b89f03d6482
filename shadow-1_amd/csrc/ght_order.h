// ght_order.h -- the order in which GLib's GHashTable hands out its entries,
// for a table keyed by small integers under g_direct_hash (plain C++, host).
//
// The reference keeps a socket's retransmit queue in such a table keyed by
// the segment's sequence (tcp.c:854-874), and _tcp_clearRetransmit
// (tcp.c:876-897) walks it with a GHashTableIter: the [STATUS] lines of the
// segments a closing socket drops come in the table's order, which depends on
// the table's whole history of inserts, removals and resizes.  This restates
// what that order needs of ghash.c as of GLib 2.58 .. 2.72 (open addressing,
// triangular probing, tombstones, the hash multiplied by 11 before the modulo,
// resizing in place by eviction chains): the hash and key arrays, nothing of
// the values.  tests/test_tcp_hub_ref_cpu.py runs it against the system's
// GLib on random histories.
#ifndef SHD_GHT_ORDER_H
#define SHD_GHT_ORDER_H

#include <stdint.h>

#include <vector>

struct GhtOrder {
    std::vector<uint32_t> hashes, keys;   // hashes: 0 unused, 1 tombstone, >= 2 the entry's hash
    uint32_t shift = 0, size = 0, mod = 0, mask = 0;
    int32_t nnodes = 0, noccupied = 0;

    GhtOrder() { set_shift(3); hashes.assign(size, 0); keys.assign(size, 0); }   // HASH_TABLE_MIN_SHIFT

    static uint32_t prime_mod(uint32_t s) {
        static const uint32_t p[] = {1, 2, 3, 7, 13, 31, 61, 127, 251, 509, 1021, 2039, 4093, 8191, 16381, 32749, 65521,
                                     131071, 262139, 524287, 1048573, 2097143, 4194301, 8388593, 16777213, 33554393,
                                     67108859, 134217689, 268435399, 536870909, 1073741789, 2147483647};
        return p[s];
    }
    void set_shift(uint32_t s) { shift = s; size = 1u << s; mod = prime_mod(s); mask = size - 1; }
    void set_shift_from_size(int32_t n) {   // g_hash_table_find_closest_shift: the bits of n
        uint32_t s = 0;
        for (; n; s++) n >>= 1;
        set_shift(s < 3 ? 3 : s);
    }
    static uint32_t hash_of(uint32_t key) { return key < 2 ? 2 : key; }   // g_direct_hash, made HASH_IS_REAL
    uint32_t to_index(uint32_t hash) const { return (hash * 11u) % mod; }

    uint32_t lookup(uint32_t key) const {   // g_hash_table_lookup_node
        const uint32_t hv = hash_of(key);
        uint32_t i = to_index(hv), first_tomb = 0, step = 0;
        bool have_tomb = false;
        while (hashes[i] != 0) {
            if (hashes[i] == hv && keys[i] == key) return i;
            if (hashes[i] == 1 && !have_tomb) { first_tomb = i; have_tomb = true; }
            step++;
            i = (i + step) & mask;
        }
        return have_tomb ? first_tomb : i;
    }
    void resize() {   // g_hash_table_resize: in place, entries moved along eviction chains
        const uint32_t old_size = size;
        set_shift_from_size((int32_t)((double)nnodes * 1.333));
        if (size > old_size) { hashes.resize(size, 0); keys.resize(size, 0); }
        std::vector<uint8_t> moved(size > old_size ? size : old_size, 0);
        for (uint32_t i = 0; i < old_size; i++) {
            uint32_t h = hashes[i];
            if (h < 2) { hashes[i] = 0; continue; }   // tombstones go
            if (moved[i]) continue;
            hashes[i] = 0;
            uint32_t key = keys[i];
            for (;;) {
                uint32_t at = to_index(h), step = 0;
                while (moved[at]) { step++; at = (at + step) & mask; }
                moved[at] = 1;
                const uint32_t rh = hashes[at], rk = keys[at];
                hashes[at] = h;
                keys[at] = key;
                if (rh < 2) break;
                h = rh;
                key = rk;
            }
        }
        if (size < old_size) { hashes.resize(size); keys.resize(size); }
        noccupied = nnodes;
    }
    void maybe_resize() {
        if (((int32_t)size > nnodes * 4 && size > 8) || (int32_t)size <= noccupied + noccupied / 16) resize();
    }
    void insert(uint32_t key) {   // g_hash_table_insert of a key that may be present
        const uint32_t i = lookup(key), old = hashes[i];
        hashes[i] = hash_of(key);
        keys[i] = key;
        if (old >= 2) return;
        nnodes++;
        if (old == 0) { noccupied++; maybe_resize(); }
    }
    // g_hash_table_remove / _steal (resize considered) or g_hash_table_iter_remove (not)
    void remove(uint32_t key, bool iter) {
        const uint32_t i = lookup(key);
        if (hashes[i] < 2) return;
        hashes[i] = 1;
        nnodes--;
        if (!iter) maybe_resize();
    }
    // the keys as a GHashTableIter meets them
    void order(std::vector<uint32_t>& out) const {
        out.clear();
        for (uint32_t i = 0; i < size; i++)
            if (hashes[i] >= 2) out.push_back(keys[i]);
    }
};

#endif
