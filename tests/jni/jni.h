/*
 * A STAND-IN jni.h FOR THE TESTS OF bindings/jni/needle_jni.c -- NOT A JVM'S HEADER.
 *
 * Written for this project from the names of the JNI specification: the primitive and reference types, the
 * calling-convention macros, the release modes, and a function table that holds exactly the members the shim uses, IN
 * AN ORDER OF ITS OWN.  A JVM's struct JNINativeInterface_ has some 230 members in a fixed order; a library compiled
 * against THIS header calls the wrong slots of a real JNIEnv.  Whatever is built with it (tests/jni/fake_jvm.c and the
 * shim, as one libneedle_jni_fake.so or one test program) is for these tests only and must never be loaded by a JVM.
 *
 * As in a JDK's header under C, every reference type is the same pointer type, so a jintArray passes where a jarray is
 * expected without a cast and the shim sees the conversions a real build would see.
 */
#ifndef NEEDLE_TESTS_STAND_IN_JNI_H
#define NEEDLE_TESTS_STAND_IN_JNI_H

#include <stdint.h>

typedef unsigned char jboolean;
typedef signed char jbyte;
typedef unsigned short jchar;
typedef short jshort;
typedef int32_t jint;
typedef int64_t jlong;
typedef float jfloat;
typedef double jdouble;
typedef jint jsize;

struct _jobject;
typedef struct _jobject *jobject;
typedef jobject jclass;
typedef jobject jstring;
typedef jobject jarray;
typedef jarray jobjectArray;
typedef jarray jbooleanArray;
typedef jarray jbyteArray;
typedef jarray jcharArray;
typedef jarray jshortArray;
typedef jarray jintArray;
typedef jarray jlongArray;
typedef jarray jfloatArray;
typedef jarray jdoubleArray;

#define JNI_FALSE 0
#define JNI_TRUE 1
#define JNI_COMMIT 1
#define JNI_ABORT 2

#define JNIEXPORT __attribute__((visibility("default")))
#define JNIIMPORT
#define JNICALL

struct JNINativeInterface_;
typedef const struct JNINativeInterface_ *JNIEnv;

struct JNINativeInterface_ {
    jstring (*NewStringUTF)(JNIEnv *env, const char *utf);
    jsize (*GetArrayLength)(JNIEnv *env, jarray array);
    jboolean (*ExceptionCheck)(JNIEnv *env);
    jobject (*GetObjectArrayElement)(JNIEnv *env, jobjectArray array, jsize index);
    void *(*GetDirectBufferAddress)(JNIEnv *env, jobject buf);
    jbyteArray (*NewByteArray)(JNIEnv *env, jsize len);

    jbyte *(*GetByteArrayElements)(JNIEnv *env, jbyteArray array, jboolean *isCopy);
    jchar *(*GetCharArrayElements)(JNIEnv *env, jcharArray array, jboolean *isCopy);
    jshort *(*GetShortArrayElements)(JNIEnv *env, jshortArray array, jboolean *isCopy);
    jint *(*GetIntArrayElements)(JNIEnv *env, jintArray array, jboolean *isCopy);
    jlong *(*GetLongArrayElements)(JNIEnv *env, jlongArray array, jboolean *isCopy);

    void (*ReleaseByteArrayElements)(JNIEnv *env, jbyteArray array, jbyte *elems, jint mode);
    void (*ReleaseCharArrayElements)(JNIEnv *env, jcharArray array, jchar *elems, jint mode);
    void (*ReleaseShortArrayElements)(JNIEnv *env, jshortArray array, jshort *elems, jint mode);
    void (*ReleaseIntArrayElements)(JNIEnv *env, jintArray array, jint *elems, jint mode);
    void (*ReleaseLongArrayElements)(JNIEnv *env, jlongArray array, jlong *elems, jint mode);

    void (*SetIntArrayRegion)(JNIEnv *env, jintArray array, jsize start, jsize len, const jint *buf);
    void (*SetLongArrayRegion)(JNIEnv *env, jlongArray array, jsize start, jsize len, const jlong *buf);
    void (*SetFloatArrayRegion)(JNIEnv *env, jfloatArray array, jsize start, jsize len, const jfloat *buf);
    void (*GetIntArrayRegion)(JNIEnv *env, jintArray array, jsize start, jsize len, jint *buf);
};

#endif
