/* Empty stand-in: the reference's inc/global.h and LKRefine/LKSubPixel.h include
 * this header, and src/{Solver,SGM,cost,BM}.cpp use nothing from it.
 * Test infrastructure only (oracle/Makefile, target ref). */
