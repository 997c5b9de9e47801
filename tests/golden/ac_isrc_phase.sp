* AC current source with a phase into R || C; a second AC source (voltage, -90 degrees) through a resistor
I1 a 0 DC 1m AC 2 30
R1 a 0 1k
C1 a 0 1n
V2 b 0 AC 0.5 -90
R2 b a 2k
.AC DEC 5 1k 10meg
