// GhtOrder against the system's GLib on random histories of a sliding window of keys
#include <stdio.h>
#include <stdlib.h>
#include "ght_order.h"
extern "C" {
typedef struct _GHashTable GHashTable;
typedef struct { void* a; void* b; void* c; int d; int e; void* f; } GHashTableIter;
GHashTable* g_hash_table_new(void*, void*);
int g_hash_table_insert(GHashTable*, void*, void*);
int g_hash_table_remove(GHashTable*, const void*);
int g_hash_table_steal(GHashTable*, const void*);
void g_hash_table_iter_init(GHashTableIter*, GHashTable*);
int g_hash_table_iter_next(GHashTableIter*, void**, void**);
void g_hash_table_iter_remove(GHashTableIter*);
void g_hash_table_destroy(GHashTable*);
}
static uint32_t rs = 12345;
static uint32_t rnd() { rs = rs * 1103515245u + 12345u; return rs >> 8; }
int main() {
    long checks = 0;
    for (int trial = 0; trial < 300; trial++) {
        GHashTable* t = g_hash_table_new(nullptr, nullptr);   // g_direct_hash, g_direct_equal
        GhtOrder o;
        std::vector<uint32_t> live, ord;
        uint32_t next = trial % 3 == 0 ? 0 : 1;
        const uint32_t width = 1 + rnd() % (trial % 7 == 0 ? 3000 : 200);
        for (int op = 0; op < 4000; op++) {
            const uint32_t r = rnd() % 100;
            if (r < 45 && live.size() < width) {   // the next sequence, or one sent again
                uint32_t k = next++;
                if (r < 3 && !live.empty()) k = live[rnd() % live.size()];
                g_hash_table_insert(t, (void*)(uintptr_t)k, (void*)1);
                o.insert(k);
                bool has = false;
                for (uint32_t x : live) has |= x == k;
                if (!has) live.push_back(k);
            } else if (r < 85 && !live.empty()) {   // acknowledged from the front, or any (a SACKed range, a steal)
                const size_t j = r < 70 ? 0 : rnd() % live.size();
                const uint32_t k = live[j];
                if (r & 1) g_hash_table_remove(t, (void*)(uintptr_t)k); else g_hash_table_steal(t, (void*)(uintptr_t)k);
                o.remove(k, false);
                live.erase(live.begin() + j);
            } else if (r < 88) {   // a clear below some sequence through an iterator
                const uint32_t below = live.empty() ? 1 : live[rnd() % live.size()] + (rnd() & 1);
                o.order(ord);
                GHashTableIter it;
                void *k, *v;
                g_hash_table_iter_init(&it, t);
                size_t i = 0;
                while (g_hash_table_iter_next(&it, &k, &v)) {
                    if (i >= ord.size() || ord[i] != (uint32_t)(uintptr_t)k) { printf("order differs: trial %d op %d\n", trial, op); return 1; }
                    i++;
                    if ((uint32_t)(uintptr_t)k < below) {
                        g_hash_table_iter_remove(&it);
                        o.remove((uint32_t)(uintptr_t)k, true);
                        for (size_t j = 0; j < live.size(); j++) if (live[j] == (uint32_t)(uintptr_t)k) { live.erase(live.begin() + j); break; }
                    }
                }
                if (i != ord.size()) { printf("count differs: trial %d op %d\n", trial, op); return 1; }
                checks++;
            }
        }
        g_hash_table_destroy(t);
    }
    printf("ok %ld\n", checks);
    return 0;
}
