/*
 * bindings/jni/needle_jni.c under AddressSanitizer and UBSan, without a JVM and without Python in the process: this program, the
 * shim and tests/jni/fake_jvm.c are compiled with -fsanitize=address,undefined -fno-sanitize-recover=all (libneedle_hip.so is linked
 * as it is) and run the script tests/test_jni_shim.py writes to stdin -- the device-free natives with the values the ctypes path
 * gave, and every argument-validation case (tests/jni_shim_cases.py: ops_text() documents the lines).  Exit status 0: every
 * expectation held; the sanitizers abort the program themselves.
 *
 * jni_shim_dispatch.inc is written by the test from Native.java's declarations: a prototype and one call line per native.
 */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fake_jvm.h"

typedef struct {
    jobject o;
    long long n;
} arg;

#define MAX_IDS (1 << 17)
static jobject g_objs[MAX_IDS];
static void *g_memory[MAX_IDS]; /* under the direct buffers */
static size_t g_n_memory;
static char g_label[512];
static int g_failures, g_faults_seen;
static long g_line;

static void fail(const char *what) {
    g_failures++;
    fprintf(stderr, "line %ld [%s]: %s | faults: %s\n", g_line, g_label, what, fj_fault_log());
}

static size_t unhex(const char *hex, unsigned char *out) {
    if (!hex || !strcmp(hex, "-")) return 0;
    size_t n = strlen(hex) / 2;
    for (size_t i = 0; i < n; i++) {
        unsigned v;
        sscanf(hex + 2 * i, "%2x", &v);
        out[i] = (unsigned char)v;
    }
    return n;
}

static jobject obj(const char *tok) {
    long id = strtol(tok, NULL, 10);
    if (id < 0 || id >= MAX_IDS || !g_objs[id]) {
        fprintf(stderr, "line %ld: no object %ld\n", g_line, id);
        exit(2);
    }
    return g_objs[id];
}

/* the next token of the line; a script that ends early is the script's fault, not the shim's */
static const char *token(char **save) {
    const char *t = strtok_r(NULL, " \n", save);
    if (!t) {
        fprintf(stderr, "line %ld: the line ends early\n", g_line);
        exit(2);
    }
    return t;
}

static long number(char **save) { return strtol(token(save), NULL, 10); }

/* the id a new object gets: inside the table */
static long new_id(char **save) {
    long id = number(save);
    if (id < 0 || id >= MAX_IDS) {
        fprintf(stderr, "line %ld: id %ld outside 0 .. %d\n", g_line, id, MAX_IDS - 1);
        exit(2);
    }
    return id;
}

static jlong first_long(jobject a) {
    jlong v = 0;
    if (fj_array_bytes(a) >= sizeof(v)) memcpy(&v, fj_array_data(a), sizeof(v));
    return v;
}

/* what the last call returned */
static long long r_int;
static jobject r_obj;

#define R_INT(call) (r_int = (long long)(call), r_obj = NULL)
#define R_OBJ(call) (r_obj = (call), r_int = 0)
#define R_VOID(call) ((call), r_int = 0, r_obj = NULL)
#include "jni_shim_dispatch.inc" /* static int dispatch(JNIEnv *env, const char *name, int argc, const arg *a): 0 when there is no such native */

int main(void) {
    char *line = NULL;
    size_t cap = 0;
    long ops = 0;
    JNIEnv *env = fj_env();
    unsigned char *bytes = NULL;
    while (getline(&line, &cap, stdin) > 0) {
        g_line++;
        bytes = (unsigned char *)realloc(bytes, strlen(line) / 2 + 8);
        if (!bytes) return 2;
        char *save = NULL;
        char *op = strtok_r(line, " \n", &save);
        if (!op) continue;
        ops++;
        if (!strcmp(op, "label")) {
            size_t n = unhex(token(&save), bytes);
            if (n >= sizeof(g_label)) n = sizeof(g_label) - 1;
            memcpy(g_label, bytes, n);
            g_label[n] = 0;
        } else if (!strcmp(op, "array")) {
            long id = new_id(&save);
            int kind = (int)number(&save);
            long len = number(&save);
            size_t have = unhex(token(&save), bytes);
            if (len < 0 || kind < FJ_BYTE || kind > FJ_FLOAT || have != (size_t)len * (kind == FJ_BYTE ? 1 : kind == FJ_LONG ? 8 : kind <= FJ_SHORT ? 2 : 4)) {
                fprintf(stderr, "line %ld: an array of %ld elements of kind %d with %zu bytes\n", g_line, len, kind, have);
                return 2;
            }
            g_objs[id] = fj_new_array(kind, (jsize)len, bytes);
        } else if (!strcmp(op, "objects") || !strcmp(op, "gather")) {
            long id = new_id(&save);
            long n = number(&save);
            if (n < 0 || n > MAX_IDS) return 2;
            jobject *els = (jobject *)calloc((size_t)n + 1, sizeof(jobject));
            jlong *vals = (jlong *)calloc((size_t)n + 1, sizeof(jlong));
            if (!els || !vals) return 2;
            for (long i = 0; i < n; i++) {
                const char *t = token(&save);
                els[i] = strcmp(t, "-") ? obj(t) : NULL;
                vals[i] = els[i] && op[0] == 'g' ? first_long(els[i]) : 0;
            }
            g_objs[id] = op[0] == 'g' ? fj_new_array(FJ_LONG, (jsize)n, vals) : fj_new_object_array((jsize)n, els);
            free(els);
            free(vals);
        } else if (!strcmp(op, "buffer")) {
            long id = new_id(&save);
            long n = number(&save);
            const char *hex = token(&save);
            if (n < 0 || g_n_memory >= MAX_IDS || (strcmp(hex, "-") ? strlen(hex) / 2 : 0) != (size_t)n) return 2;
            void *m = malloc((size_t)n + 1);
            if (!m) return 2;
            unhex(hex, (unsigned char *)m);
            g_memory[g_n_memory++] = m;
            g_objs[id] = fj_new_direct_buffer(m, n);
        } else if (!strcmp(op, "heap_buffer")) {
            g_objs[new_id(&save)] = fj_new_heap_buffer();
        } else if (!strcmp(op, "call")) {
            char name[64];
            arg a[16];
            snprintf(name, sizeof(name), "%s", token(&save));
            int argc = (int)number(&save);
            if (argc > 16) return 2;
            for (int i = 0; i < argc; i++) {
                const char *t = token(&save);
                a[i].o = NULL;
                a[i].n = 0;
                if (t[0] == '@') a[i].o = obj(t + 1);
                else if (t[0] == '#') a[i].n = strtoll(t + 1, NULL, 10);
                else if (t[0] == '*') a[i].n = first_long(obj(t + 1));
            }
            fj_clear_exception(); /* Java code runs between two natives: nothing is pending when one is entered */
            if (!dispatch(env, name, argc, a)) {
                fprintf(stderr, "line %ld: no native %s with %d arguments\n", g_line, name, argc);
                return 2;
            }
        } else if (!strcmp(op, "ret")) {
            long long want = strtoll(token(&save), NULL, 10);
            if (r_int != want) {
                char msg[96];
                snprintf(msg, sizeof(msg), "returned %lld, expected %lld", r_int, want);
                fail(msg);
            }
        } else if (!strcmp(op, "ret_null")) {
            if (r_obj) fail("returned an object, expected null");
        } else if (!strcmp(op, "ret_string")) {
            size_t n = unhex(token(&save), bytes);
            const char *s = fj_string_utf(r_obj);
            if (!s || strlen(s) != n || memcmp(s, bytes, n)) fail("the returned String differs");
        } else if (!strcmp(op, "ret_bytes")) {
            size_t n = unhex(token(&save), bytes);
            if (!r_obj || fj_array_bytes(r_obj) != n || memcmp(fj_array_data(r_obj), bytes, n)) fail("the returned byte[] differs");
        } else if (!strcmp(op, "bytes")) {
            jobject a = obj(token(&save));
            size_t n = unhex(token(&save), bytes);
            if (fj_array_bytes(a) != n || (n && memcmp(fj_array_data(a), bytes, n))) fail("an array does not hold the expected bytes");
        } else if (!strcmp(op, "nonzero") || !strcmp(op, "zero")) {
            jlong v = first_long(obj(token(&save)));
            if ((v != 0) != (op[0] == 'n')) fail(op[0] == 'n' ? "a handle is 0" : "a handle is not 0");
        } else if (!strcmp(op, "clean")) {
            if (fj_outstanding_pins()) fail("Get...Elements without a release");
            if (fj_fault_count(-1) != g_faults_seen) fail("the fake JVM recorded a fault");
            g_faults_seen = fj_fault_count(-1); /* (one fault fails one case, not every case behind it) */
        } else if (!strcmp(op, "fail_gets")) {
            int skip = (int)number(&save);
            fj_fail_gets(skip, (int)number(&save));
        } else if (!strcmp(op, "fail_consumed")) {
            if (fj_fail_gets_left()) fail("the native made fewer Get...Elements calls than the case expects");
            fj_fail_gets(0, 0);
        } else {
            fprintf(stderr, "line %ld: unknown op %s\n", g_line, op);
            return 2;
        }
        if (g_failures > 20) break;
    }
    free(line);
    free(bytes);
    fj_reset();
    for (size_t i = 0; i < g_n_memory; i++) free(g_memory[i]);
    if (g_failures) return 1;
    printf("jni shim check ok: %ld ops\n", ops);
    return 0;
}
